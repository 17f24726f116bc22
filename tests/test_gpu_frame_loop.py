"""The deferred frame loop end to end on the GPU: the README's "whole frame loop", written as the README prints it,
against the sequential host replay of tests/frame_loop_reference.py. Tolerance 0: every pass equals its twin bit for
bit, so the composition of passes equals the composition of twins bit for bit. Every plane, every pixel and every
compared frame is checked; nothing is masked.

Scene REFLO at 37 x 21 (partial 8 x 8 tiles and partial workgroups), displayed at 74 x 42, under
test_gpu_reflection_chain's MIRRORS table. Script, 6 frames: the camera orbits one manipulator step per frame with
Halton jitter, instance 1 is translated every frame, the teapot mesh is deformed before frames 2 and 4 (rt_blas_refit,
test_gpu_motion.displaced, then rt_tlas_build(update_only)), motion history is on from before the first build. Passes:
S = 1 everywhere, shadow light_radius 0.5, AO radius 2, the mirror chain with max_bounces 4 and RT_REFLECT_FRAME_RAY,
indirect with RT_REFLECT_SHADOW_MODELS, three a-trous iterations, max_history 4.

After every frame every plane is copied device to device, on the stream that wrote it, into a per-frame log; the host
synchronises once, after the last frame. Every buffer is pre-filled with 0xAB bytes and followed by a guard region.

The expected planes come from frame_loop_reference.replay: the trace half from the CPU oracle's searches (under the
watertight test: Context.trace_rays on a second context, synchronised after every call), never from the passes under
test; computed once per module and shared.

Which branch of the context's lifetime machinery each test reaches (rt_api.cpp) is said in its docstring. The tests
check results; a wrong ordering shows as a differing plane.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402

import frame_loop_reference as fl  # noqa: E402
from test_gpu_materials import map_tensor  # noqa: E402
from test_gpu_motion import displaced, shifted  # noqa: E402
from test_gpu_reflection import any_hit, closest  # noqa: E402
from test_gpu_reflection_chain import IMAP, MIRRORS  # noqa: E402
from test_gpu_shadow import FILL, GUARD, LANE, MT, PACKET, WT, filled, spec_of  # noqa: E402

W, H, DW, DH, FRAMES = 37, 21, 74, 42, 6
N, ND = W * H, DW * DH
REFITS = {2: 0.15, 4: -0.2}  # frame -> displaced()'s amount for the teapot mesh (mesh 0)
STEP = (0.05, 0.02, -0.03)   # instance 1's translation per frame
RT_REFLECT_FRAME_RAY, RT_REFLECT_SHADOW_MODELS = rt.RT_REFLECT_FRAME_RAY, rt.RT_REFLECT_SHADOW_MODELS
# the logged planes, in the loop's order (a failure names the first frame and plane that differ): name, words
LOGGED = (("hits", 4 * N), ("normal", 4 * N), ("object", 2 * N), ("motion", 4 * N), ("vis_raw", None), ("guide", 4 * N),
          ("vis_acc", None), ("vhist", None), ("vis_flt", None), ("ao_raw", N), ("ao_acc", N), ("hist", N),
          ("ao_flt", N), ("refl", 4 * N), ("rmotion", 4 * N), ("racc", 4 * N), ("rmom", 4 * N), ("refl_flt", 4 * N),
          ("refl_var", N), ("ind", 4 * N), ("iacc", 4 * N), ("imom", 4 * N), ("ind_flt", 4 * N), ("ind_var", N),
          ("color", 4 * N), ("out", 4 * ND), ("hist_up", ND), ("rgba8", ND))

_EXPECT = {}


# ---- the scripts and their replays (computed once per module) ------------------------------------------------------
def reflo_script(frames=FRAMES, moving=True):
    """The issue's script; moving False: the cameras alone (a static scene: no TLAS update between the frames)."""
    base = spec_of("REFLO", W, H)
    cbs, js = fl.jittered(fl.orbit_cameras(base, frames), W, H)
    specs, verts = [], {}
    for k in range(frames):
        if moving and k in REFITS:
            verts = {0: displaced(base.meshes[0][0], REFITS[k])}
        xf = None
        if moving:
            xf = [shifted(x, [k * d for d in STEP]) if i == 1 else x for i, (_, x, _, _) in enumerate(base.instances)]
        specs.append(fl.frame_spec(base, cbs[k], xf, verts))
    return fl.Script(W, H, DW, DH, specs, js, list(range(frames)), MIRRORS, IMAP)


def deep_script(frames=2):
    """DEEP (stack_cap > lds_cap: the per-lane kernels need the HBM overflow stack) at 37 x 21, a static scene under
    the orbit; every model instance reflects."""
    base = spec_of("DEEP", W, H)
    cbs, js = fl.jittered(fl.orbit_cameras(base, frames), W, H)
    return fl.Script(W, H, DW, DH, [fl.frame_spec(base, cb) for cb in cbs], js, list(range(frames)), MIRRORS,
                     np.array([0, 1, 3, 2], np.uint32))


class LibraryTracers:
    """Context.trace_rays' searches (pinned to brute force by tests/test_gpu_random_scenes.py) of one frame's scene on
    a context of its own, under triangle test tt; test_gpu_reflection's helpers synchronise after every call."""

    def __init__(self, c, spec):
        self.c, self.spec = c, spec

    def primary(self, rays):
        return closest(self.c, self.spec, rays, True, cull=False)

    def closest(self, rays):
        return closest(self.c, self.spec, rays, True)

    def any_hit(self, rays):
        return any_hit(self.c, self.spec, rays, True)


def raw_planes(name, script, tt=MT):
    """The trace half of every frame of a script, once per (script, triangle test)."""
    key = ("raw", name, tt)
    if key not in _EXPECT:
        raw = []
        for k, spec in enumerate(script.frames):
            if tt == MT:
                raw.append(fl.trace_frame(script, k, fl.OracleTracers(spec)))
            else:
                with rt.Context(0) as c2:
                    scenes.upload(c2, spec)
                    c2.set_triangle_test(tt)
                    raw.append(fl.trace_frame(script, k, LibraryTracers(c2, spec)))
        _EXPECT[key] = raw
    return _EXPECT[key]


def expected(name, script, tt=MT):
    key = ("replay", name, tt)
    if key not in _EXPECT:
        _EXPECT[key] = fl.replay(script, raw_planes(name, script, tt))
    return _EXPECT[key]


# ---- device buffers ------------------------------------------------------------------------------------------------
class Buffers:
    """Pre-filled, guarded device buffers by name; attribute access gives the plane's view."""

    def __init__(self):
        self._all = {}

    def add(self, name, shape, dtype=torch.float32):
        words = int(np.prod(shape))
        t = filled(words + GUARD, dtype)
        self._all[name] = t
        setattr(self, name, t[:words].view(*shape))

    def guards_intact(self, what):
        for name, t in self._all.items():
            tail = t[-GUARD:].cpu().numpy().view(np.uint32)
            assert (tail == FILL).all(), f"{what}: the guard region after {name} was written"


def planes(L):
    """One side of the ping-pong: hits, normal, motion, guide, color, refl, rmotion, racc, rmom, ind, iacc, imom
    (n x 4); object (n x 2); vis, vhist (L x n); ao, hist (n); out (N x 4), hist_up (N)."""
    g = Buffers()
    g.add("hits", (N, 4), torch.int32)
    g.add("object", (N, 2), torch.int32)
    for name in ("normal", "motion", "guide", "color", "refl", "rmotion", "racc", "rmom", "ind", "iacc", "imom"):
        g.add(name, (N, 4))
    g.add("vis", (L, N))
    g.add("vhist", (L, N))
    g.add("ao", (N,))
    g.add("hist", (N,))
    g.add("out", (ND, 4))
    g.add("hist_up", (ND,))
    return g


def shared(L):
    """What is not ping-ponged: the filtered planes the resolve reads, the filters' scratch, the display frame."""
    s = Buffers()
    s.add("shown_vis", (L, N))
    for name in ("shown_ao", "tmp", "tmp_b", "rvar", "rvtmp", "ivar", "ivtmp"):
        s.add(name, (N,))
    for name in ("shown_refl", "rtmp", "shown_ind", "itmp", "spare", "spare2"):
        s.add(name, (N, 4))
    s.add("shown32", (ND,), torch.int32)
    s.shown = s.shown32.view(torch.uint8).view(DH, DW, 4)
    return s


def frame_log(L, frames):
    log = Buffers()
    for name, words in LOGGED:
        log.add(name, (frames, L * N if words is None else words), torch.int32)
    return log


def keep(log, k, name, src, stream):
    """Device-to-device copy of a plane into frame k's log entry on `stream`; no host synchronisation."""
    with torch.cuda.stream(stream):
        getattr(log, name)[k].copy_(src.reshape(-1).view(torch.int32) if src.dtype != torch.uint8
                                    else src.view(torch.int32).reshape(-1))


# ---- the loop, as the README prints it -----------------------------------------------------------------------------
class Loop:
    """The context, the ping-pong planes and the log of one run of the README's loop. A: the stream of the G-buffer,
    shadow, reflection, resolve and upscale passes; B: the stream of the AO and indirect chains (A itself unless the
    test joins two streams by PipelineEvents)."""

    def __init__(self, script, A, B=None, schedule=None, tt=MT):
        self.script, self.A, self.B = script, A, A if B is None else B
        self.L = len(script.frames[0].lights)
        c = self.c = rt.Context(0)
        c.set_motion_history(True)  # from before the first build
        self.ids = scenes.upload(c, script.frames[0])
        c.set_shading(script.frames[0].lights, script.frames[0].material, rt.RT_SHADE_REF, 1)
        if schedule is not None:
            c.set_schedule(schedule)
        c.set_triangle_test(tt)
        self.imap = map_tensor(script.imap)
        with torch.cuda.stream(self.A):
            self.g, self.prev, self.sh = planes(self.L), planes(self.L), shared(self.L)
            self.log = frame_log(self.L, len(script.frames))
        self.events = (rt.PipelineEvent(), rt.PipelineEvent()) if self.B is not self.A else None
        torch.cuda.synchronize()  # the fills are done; from here on the host waits only after the last frame
        self.enqueue_s = []

    def update_scene(self, k):
        """Frame k's geometry: the refit of the teapot mesh (it quiesces by design), then the TLAS update."""
        cur, before = self.script.frames[k], self.script.frames[k - 1]
        if cur.meshes[0][0] is not before.meshes[0][0]:
            self.c.blas_refit(self.ids[0], cur.meshes[0][0])
        moved = any((x != y).any() for (_, x, _, _), (_, y, _, _) in zip(cur.instances, before.instances))
        if moved or cur.meshes[0][0] is not before.meshes[0][0]:
            self.c.tlas_build([(self.ids[m], x, iid, hg) for (m, x, iid, hg) in cur.instances], update_only=True)

    def frame(self, frame, refused_call=False):
        """One frame of the README's loop (README.md, "The whole frame loop"): its method names, keyword arguments,
        in-place forms and ping-pong, every optional pass switched on."""
        c, s, g, prev, sh, log = self.c, self.script, self.g, self.prev, self.sh, self.log
        w, h, L, materials, imap = W, H, self.L, s.materials, self.imap
        A, B = self.A, self.B
        a, b = A.cuda_stream, B.cuda_stream
        cbj, j = s.frames[frame].cb, s.jitters[frame]
        prev_cbj, prev_j = (s.frames[frame - 1].cb, s.jitters[frame - 1]) if frame else (None, (0.0, 0.0))
        seed = s.seeds[frame]
        t0 = time.perf_counter()
        c.set_camera(cbj)
        c.dispatch_gbuffer_motion(w, h, hits=g.hits, normal=g.normal, object=g.object, motion=g.motion,
                                  prev_camera=prev_cbj, stream=a)
        c.dispatch_shadow(w, h, g.vis, samples=1, light_radius=0.5, seed=seed, stream=a)
        keep(log, frame, "vis_raw", g.vis, A)
        c.denoise_guide(w * h, g.normal, g.motion.view(-1)[3:], g.guide, stream=a)
        if self.events:  # B's chains read the G-buffer, the motion plane and the guide
            self.events[0].record(a)
            self.events[0].wait_on(b)
        for l in range(L):  # each light's plane through the AO filter, in place
            hist = (prev.vis[l], prev.vhist[l], prev.guide) if frame else (None, None, None)
            c.ao_accumulate(w, h, g.vis[l], g.motion, g.guide, g.vis[l], g.vhist[l], *hist, max_history=4, stream=a)
            c.ao_atrous(w, h, g.vis[l], g.guide, sh.shown_vis[l], sh.tmp, iterations=3, stream=a)
        c.dispatch_ao(w, h, g.ao, samples=1, radius=2.0, seed=seed, stream=b)
        keep(log, frame, "ao_raw", g.ao, B)
        history = (prev.ao, prev.hist, prev.guide) if frame else (None, None, None)
        c.ao_accumulate(w, h, g.ao, g.motion, g.guide, g.ao, g.hist, *history, max_history=4, stream=b)  # in place
        c.ao_atrous(w, h, g.ao, g.guide, sh.shown_ao, sh.tmp_b if self.events else sh.tmp, iterations=3, stream=b)
        c.dispatch_reflection_chain(w, h, g.refl, materials, imap, samples=1, roughness=0.0, seed=seed,
                                    flags=RT_REFLECT_FRAME_RAY, max_bounces=4, stream=a)
        c.reflection_motion(w, h, g.hits, g.guide, g.motion, g.refl.view(-1)[3:], cbj, prev_cbj if frame else cbj,
                            g.rmotion, guide_prev=prev.guide if frame else None, stream=a)
        rhist = (prev.racc, prev.rmom, prev.guide) if frame else (None, None, None)
        c.radiance_accumulate(w, h, g.refl, g.rmotion, g.guide, g.racc, g.rmom, *rhist, max_history=4, stream=a)
        if refused_call:  # a misaligned plane pointer: refused, nothing written, the loop goes on
            with pytest.raises(rt.RtError) as e:
                c.radiance_accumulate(w, h, g.refl, g.rmotion, g.guide, sh.spare.data_ptr() + 4, sh.spare2, *rhist,
                                      max_history=4, stream=a)
            assert e.value.status == rt.RT_E_INVALID, str(e.value)
            with pytest.raises(rt.RtError) as e:  # no previous camera buffer: what a first frame must not pass
                c.reflection_motion(w, h, g.hits, g.guide, g.motion, g.refl.view(-1)[3:], cbj, None, sh.spare, stream=a)
            assert e.value.status == rt.RT_E_INVALID, str(e.value)
        c.radiance_atrous(w, h, g.racc, g.rmom, g.guide, sh.shown_refl, sh.rvar, sh.rtmp, sh.rvtmp, iterations=3, stream=a)
        c.dispatch_indirect(w, h, g.ind, materials, imap, samples=1, seed=seed, flags=RT_REFLECT_SHADOW_MODELS, stream=b)
        ihist = (prev.iacc, prev.imom, prev.guide) if frame else (None, None, None)
        c.radiance_accumulate(w, h, g.ind, g.motion, g.guide, g.iacc, g.imom, *ihist, max_history=4, stream=b)
        c.radiance_atrous(w, h, g.iacc, g.imom, g.guide, sh.shown_ind, sh.ivar, sh.itmp, sh.ivtmp, iterations=3, stream=b)
        if self.events:  # the resolve reads B's filtered planes
            self.events[1].record(b)
            self.events[1].wait_on(a)
        c.shade_resolve_gi(w, h, g.hits, g.normal, g.object, g.color, materials, instance_material=imap,
                           vis=sh.shown_vis, ao=sh.shown_ao, refl=sh.shown_refl, indirect=sh.shown_ind,
                           indirect_scale=1.0, stream=a)
        history = dict(motion_prev=prev.motion, color_prev=prev.out, hist_prev=prev.hist_up) if frame else {}
        c.upscale(w, h, DW, DH, g.color, g.motion, g.out, g.hist_up, rgba8_out=sh.shown, jitter_cur=j,
                  jitter_prev=prev_j, max_history=4, stream=a, **history)
        # the log: each plane on the stream that wrote it
        for name, src in (("hits", g.hits), ("normal", g.normal), ("object", g.object), ("motion", g.motion),
                          ("guide", g.guide), ("vis_acc", g.vis), ("vhist", g.vhist), ("vis_flt", sh.shown_vis),
                          ("refl", g.refl), ("rmotion", g.rmotion), ("racc", g.racc), ("rmom", g.rmom),
                          ("refl_flt", sh.shown_refl), ("refl_var", sh.rvar), ("color", g.color), ("out", g.out),
                          ("hist_up", g.hist_up), ("rgba8", sh.shown)):
            keep(log, frame, name, src, A)
        for name, src in (("ao_acc", g.ao), ("hist", g.hist), ("ao_flt", sh.shown_ao), ("ind", g.ind), ("iacc", g.iacc),
                          ("imom", g.imom), ("ind_flt", sh.shown_ind), ("ind_var", sh.ivar)):
            keep(log, frame, name, src, B)
        # (B's log copies read planes that only B writes again: B's own stream order is all they need)
        self.enqueue_s.append(time.perf_counter() - t0)
        self.g, self.prev = prev, g

    def finish(self, what):
        """The one host synchronise; then the guards, and the streams are forgotten."""
        torch.cuda.synchronize()
        for bufs in (self.g, self.prev, self.sh, self.log):
            bufs.guards_intact(what)
        for spare in (self.sh.spare, self.sh.spare2):  # the refused calls' outputs still hold the fill
            assert (spare.cpu().numpy().view(np.uint32) == FILL).all(), f"{what}: a refused call's plane was written"
        for s in {self.A.cuda_stream, self.B.cuda_stream}:
            if s:
                self.c.forget_stream(s)
        got = {name: getattr(self.log, name).cpu().numpy().view(np.uint32) for name, _ in LOGGED}
        self.c.close()
        return got


def assert_frames(got, want, frames, what):
    """Every logged plane of the given frames, every word, in the loop's order."""
    for k in frames:
        for name, _ in LOGGED:
            g = got[name][k]
            w = np.ascontiguousarray(want[(k, name)])
            w = w.view(np.uint32).reshape(-1)
            assert g.shape == w.shape, (what, k, name, g.shape, w.shape)
            bad = np.nonzero(g != w)[0]
            assert bad.size == 0, (f"{what}: frame {k}, plane {name}: {bad.size} of {g.size} words differ, first word "
                                   f"{bad[0]}: {g[bad[0]]:#x} vs {w[bad[0]]:#x}")


def run(script, A, B=None, schedule=None, tt=MT, before_frame=None, after_frame=None, refuse_at=None, what=""):
    loop = Loop(script, A, B, schedule, tt)
    for k in range(len(script.frames)):
        if k:
            loop.update_scene(k)
        if before_frame:
            before_frame(loop, k)
        loop.frame(k, refused_call=k == refuse_at)
        if after_frame:
            after_frame(loop, k)
    return loop, loop.finish(what)


# ---- holding a stream back -----------------------------------------------------------------------------------------
HAS_SLEEP = hasattr(torch.cuda, "_sleep")
_RATE = {}


def delay(units):
    """A device-side delay on torch's current stream: torch.cuda._sleep(units cycles) where the installed torch has
    it, else `units` in-place multiplications by 1 of a 256 MB tensor (allocated once, before anything is held)."""
    if HAS_SLEEP:
        torch.cuda._sleep(units)
    else:
        for _ in range(units):
            _RATE["ballast"].mul_(1.0)


def delay_units_per_second():
    """The delay's rate on this device, measured once with a pair of timing events."""
    if "rate" not in _RATE:
        if not HAS_SLEEP:
            _RATE["ballast"] = torch.ones(64 << 20, dtype=torch.float32, device="cuda")
        units = 20_000_000 if HAS_SLEEP else 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        delay(1000 if HAS_SLEEP else 2)  # warm
        torch.cuda.synchronize()
        e0.record()
        delay(units)
        e1.record()
        torch.cuda.synchronize()
        _RATE["rate"] = units / (e0.elapsed_time(e1) * 1e-3)
    return _RATE["rate"]


def hold(stream, seconds):
    """A device-side delay on `stream` -> an event recorded right after it (not complete while the stream is held)."""
    units = max(1, int(np.ceil(seconds * delay_units_per_second())))
    with torch.cuda.stream(stream):
        delay(units)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def hold_time(enqueue_s, what):
    """4 x the measured host-side enqueue time, capped at 2 s."""
    t = min(4.0 * enqueue_s, 2.0)
    print(f"{what}: enqueue {enqueue_s * 1e3:.2f} ms, hold {t * 1e3:.2f} ms")
    return t


# ---- 1 .. 4, 7: the whole loop -------------------------------------------------------------------------------------
def test_readme_loop_one_stream():
    """Everything on one non-default stream, no host synchronise for 6 frames: the in-place accumulations, the
    ping-pong, two refits and five TLAS updates (the two TlasVersions wrap three times)."""
    script = reflo_script()
    want = expected("REFLO", script)
    # the input conditions of test_frame_loop_host.py, on this script's replay: the cap is reached by frame 3 and held,
    # both variance branches in the last frame, three reflection-motion classes with "virtual" (0) among them
    hist, rhist = [want[(k, "hist")] for k in range(FRAMES)], want[(FRAMES - 1, "rmom")][:, 2]
    assert not (hist[2] == 4).any() and (hist[3] == 4).any() and (hist[5] == 4).sum() > 50 and max(h.max() for h in hist) == 4
    assert ((rhist > 0) & (rhist < 4)).sum() > 50 and (rhist >= 4).sum() > 50
    classes = {int(v) for k in range(FRAMES) for v in np.unique(want[(k, "rclass")])}
    assert 0 in classes and len(classes) >= 3, classes
    t0 = time.perf_counter()
    _, got = run(script, torch.cuda.Stream(), what="one stream")
    print(f"one stream: the loop took {time.perf_counter() - t0:.2f} s")
    assert_frames(got, want, range(FRAMES), "one stream")


def test_readme_loop_both_schedules_and_triangle_tests():
    """The same loop under RT_SCHED_LANE, and under the watertight triangle test with the packet schedule (its replay's
    searches under the same test); the last two frames are compared: they carry every earlier frame's history."""
    script = reflo_script()
    _, got = run(script, torch.cuda.Stream(), schedule=LANE, what="lane")
    assert_frames(got, expected("REFLO", script), (FRAMES - 2, FRAMES - 1), "RT_SCHED_LANE")
    want = expected("REFLO", script, WT)
    _, got = run(script, torch.cuda.Stream(), schedule=PACKET, tt=WT, what="watertight")
    assert_frames(got, want, (FRAMES - 2, FRAMES - 1), "watertight")
    mt = expected("REFLO", script)
    assert any((fl.bits(want[(FRAMES - 1, p)]) != fl.bits(mt[(FRAMES - 1, p)])).any() for p in ("hits", "out")), \
        "the two triangle tests give the same frame: the second run checks nothing new"


def test_two_streams_joined_by_events():
    """The AO chain and the indirect chain on stream B, everything else on stream A; B waits for A's G-buffer and guide
    through one PipelineEvent, A waits for B's last a-trous through another before the resolve. Both streams read the
    current TlasVersion (two entries in its reader list; note_swap_out records one event per stream at each update)."""
    script = reflo_script()
    _, got = run(script, torch.cuda.Stream(), torch.cuda.Stream(), what="two streams")
    assert_frames(got, expected("REFLO", script), range(FRAMES), "two streams")


def test_tlas_update_and_refit_under_queued_deferred_work():
    """Test 1 with the stream held back by a device-side delay before every frame's passes, so the frame's launches
    are all queued when the host goes on to the next frame's rt_blas_refit (its quiesce drains them) and
    rt_tlas_build (slot_order_after_others on the version two frames back, then note_swap_out of the current one).
    rt_blas_refit quiesces by design: this documents that the quiesce and the version hand-over give the right planes
    when work really is in flight, not that the calls stay asynchronous."""
    script = reflo_script()
    want = expected("REFLO", script)
    delay_units_per_second()  # calibrated (and synchronised) before the loop starts
    # un-held: the host-side enqueue time of a warmed frame, the slowest of frames 1 .. 5 (frame 0 is the cold one)
    warm, _ = run(script, torch.cuda.Stream(), what="warm-up")
    t = [hold_time(max(warm.enqueue_s[1:]), "queued deferred work")] * FRAMES
    held = {}

    def before(loop, k):
        held[k] = hold(loop.A, t[k])

    def after(loop, k):
        done = held[k].query()
        print(f"frame {k}: still in flight after its last enqueue: {not done}")
        assert not done, f"inconclusive: frame {k}'s delay of {t[k] * 1e3:.1f} ms ended before its last enqueue"

    _, got = run(script, torch.cuda.Stream(), before_frame=before, after_frame=after, what="held back")
    assert_frames(got, want, range(FRAMES), "held back")


def test_loop_survives_a_refused_call():
    """In frame 3 one call is refused (a misaligned plane pointer): it writes nothing and the remaining frames equal
    the replay."""
    script = reflo_script()
    loop, got = run(script, torch.cuda.Stream(), refuse_at=3, what="refused call")
    assert_frames(got, expected("REFLO", script), range(FRAMES), "refused call")


# ---- 5, 6: the scratch rings ---------------------------------------------------------------------------------------
TRACE = (("hits", 4), ("normal", 4), ("object", 2), ("motion", 4), ("ao_raw", 1), ("vis_raw", None), ("refl", 4), ("ind", 4))


def row_lists(count, seed):
    """`count` distinct row lists of 3 .. 6 rows (repeats and any order allowed, as a strip dispatch may pass them)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        rows = rng.integers(0, H, size=3 + len(out) % 4).astype(np.uint32)
        if not any(np.array_equal(rows, r) for r in out):
            out.append(rows)
    return out


def trace_outputs(L, nrows):
    b = Buffers()
    for name, words in TRACE:
        dtype = torch.int32 if name in ("hits", "object") else torch.float32
        b.add(name, (L, nrows * W) if words is None else (nrows * W, words) if words > 1 else (nrows * W,), dtype)
    return b


def trace_launches(c, script, k, rows, out, stream, imap):
    """The five trace passes of frame k over a row list, each into its own compact plane."""
    s = stream.cuda_stream
    prev_cb = script.frames[k - 1].cb if k else None
    c.dispatch_gbuffer_motion(W, H, hits=out.hits, normal=out.normal, object=out.object, motion=out.motion,
                              prev_camera=prev_cb, rows=rows, stream=s)
    c.dispatch_ao(W, H, out.ao_raw, samples=1, radius=2.0, seed=script.seeds[k], rows=rows, stream=s)
    c.dispatch_shadow(W, H, out.vis_raw, samples=1, light_radius=0.5, seed=script.seeds[k], rows=rows, stream=s)
    c.dispatch_reflection_chain(W, H, out.refl, script.materials, imap, samples=1, roughness=0.0, seed=script.seeds[k],
                                flags=RT_REFLECT_FRAME_RAY, max_bounces=4, rows=rows, stream=s)
    c.dispatch_indirect(W, H, out.ind, script.materials, imap, samples=1, seed=script.seeds[k],
                        flags=RT_REFLECT_SHADOW_MODELS, rows=rows, stream=s)


def assert_rows(out, raw, rows, what):
    out.guards_intact(what)
    for name, words in TRACE:
        got = getattr(out, name).cpu().numpy().view(np.uint32)
        full = fl.bits(raw[name])
        if words is None:
            want = full.reshape(full.shape[0], H, W)[:, rows].reshape(full.shape[0], -1)
        else:
            want = full.reshape(H, W, words)[rows].reshape(got.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: plane {name}: {bad.shape[0]} of {got.size} words differ, first {bad[0]}"


def ring_run(script, name, jobs, streams, schedule, held_s, check_at, what):
    """jobs: (frame, rows, stream index) in launch order. With held_s, every stream is held back first and the holds
    must still be in flight right before job number check_at is issued. -> host seconds spent on the jobs before
    check_at. Every plane equals the replay's rows."""
    raw = raw_planes(name, script)
    L = len(script.frames[0].lights)
    with rt.Context(0) as c:
        c.set_motion_history(True)
        scenes.upload(c, script.frames[0])
        c.set_shading(script.frames[0].lights, script.frames[0].material, rt.RT_SHADE_REF, 1)
        c.set_schedule(schedule)
        imap = map_tensor(script.imap)
        outs = []
        for (k, rows, i) in jobs:  # every output is allocated and filled before anything is held
            with torch.cuda.stream(streams[i]):
                outs.append(trace_outputs(L, len(rows)))
        delay_units_per_second()  # calibrated before anything is held
        torch.cuda.synchronize()
        holds = [hold(s, held_s) for s in streams] if held_s else []
        t0, spent, frame = time.perf_counter(), None, None
        for n, ((k, rows, i), out) in enumerate(zip(jobs, outs)):
            if n == check_at:
                spent = time.perf_counter() - t0
                if holds:
                    flying = [not ev.query() for ev in holds]
                    print(f"{what}: before job {n}: holds still in flight {flying}")
                    assert all(flying), f"inconclusive: a delay of {held_s * 1e3:.1f} ms ended before job {n}"
            if k != frame:
                c.set_camera(script.frames[k].cb)
                frame = k
            trace_launches(c, script, k, rows, out, streams[i], imap)
        torch.cuda.synchronize()
        for s in streams:
            c.forget_stream(s.cuda_stream)
        for n, ((k, rows, i), out) in enumerate(zip(jobs, outs)):
            assert_rows(out, raw[k], rows, f"{what}: job {n} (frame {k}, stream {i})")
    return spent


def test_row_list_ring_reuse():
    """ring_acquire's last branch for row lists (ensure_rows): every slot busy on other streams, the least recently
    used one reused after device-side waits (slot_order_after_others). A stream may always reuse a slot only it has
    used, so the slots must be shared: three streams launch with the same three lists per frame, new lists every frame.
    A list's slot then carries the other two streams' uses, which the holds keep in flight, so no slot is free for
    anybody: lists 1 .. 8 open the ring's 8 slots and the ninth (frame 2's third) takes the branch; the holds are
    checked to be in flight right before it. (From there the host may wait for the reused slot's upload staging.)"""
    script = reflo_script(4, moving=False)
    lists = row_lists(12, 5)
    assert len({r.tobytes() for r in lists}) == 12 > 8
    streams = [torch.cuda.Stream() for _ in range(3)]
    jobs = [(k, lists[3 * k + j], i) for k in range(4) for j in range(3) for i in range(3)]
    ninth = 8 * 3  # the first job of the ninth list
    spent = ring_run(script, "REFLO static", jobs, streams, PACKET, None, ninth, "row lists, warm-up")
    t = hold_time(spent, "row-list ring")
    ring_run(script, "REFLO static", jobs, streams, PACKET, t, ninth, "row lists")


def test_overflow_ring_reuse():
    """ring_acquire's last branch for the HBM overflow stack (ensure_overflow): on DEEP under the per-lane schedule
    every trace launch takes an overflow slot (scene_view: stack_cap = TLAS max_stack + 1 + the deepest BLAS's
    max_stack > lds_cap = 32). Overflow slots are never shared, so nine held-back streams are needed: eight open the
    ring's 8 slots, the ninth finds every slot busy and reuses the least recently used one after a device-side wait
    for its stream's last use."""
    script = deep_script()
    with rt.Context(0) as c:
        ids = scenes.upload(c, script.frames[0])
        need = c.tlas_info().max_stack + 1 + max(c.blas_info(i).max_stack for i in ids)
        print(f"DEEP: per-lane stack bound {need}, LDS part 32")
        assert need > 32, "the overflow stack is not needed: the scene reaches nothing"
    lists = row_lists(3, 6)
    streams = [torch.cuda.Stream() for _ in range(9)]
    jobs = [(1, lists[i % 3], i) for i in range(9)]  # frame 1: its motion plane has a previous camera
    spent = ring_run(script, "DEEP", jobs, streams, LANE, None, 8, "overflow stacks, warm-up")
    t = hold_time(spent, "overflow ring")
    ring_run(script, "DEEP", jobs, streams, LANE, t, 8, "overflow stacks")
