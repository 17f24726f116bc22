"""The AO filter over several planes at once (rt_host_ao_accumulate_planes, rt_host_ao_atrous_planes) without a GPU.
The batched twins run the per-pixel functions the batched kernels run (reprojection and edge-stopping weights once per
pixel, sa per plane); they must equal the per-plane twins rt.host_ao_accumulate / rt.host_ao_atrous, which
tests/test_denoise_host.py pins to a numpy restatement, word for word. Tolerance 0 throughout.

Plane p of a set takes ao_cur and ao_prev from denoise_reference.synthetic(W, H, seed=p); the motion plane, the normals,
the depths and hist_prev are seed 0's."""
import ctypes

import numpy as np
import pytest

import realtimeraytracing_gradproject_amd as rt

import denoise_reference as ref

F = np.float32
TOL, NCOS = ref.DEPTH_TOL, ref.NORMAL_COS
COUNTS = [1, 2, 7, 17]
_SETS = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[:5]}"


def plane_set(W, H):
    """The shared, read-only inputs of a size: 17 planes' cur and prev, seed 0's motion, history and guides."""
    if (W, H) not in _SETS:
        syn = ref.synthetic(W, H)
        d = dict(cur=np.stack([ref.synthetic(W, H, seed=p)["ao_cur"] for p in range(17)]),
                 prev=np.stack([ref.synthetic(W, H, seed=p)["ao_prev"] for p in range(17)]),
                 motion=syn["motion"], hist_prev=syn["hist_prev"],
                 gc=rt.host_denoise_guide(syn["normal_cur"], syn["motion"][:, 3]),
                 gp=rt.host_denoise_guide(syn["normal_prev"], syn["depth_prev"]))
        for v in d.values():
            v.setflags(write=False)
        _SETS[(W, H)] = d
    return _SETS[(W, H)]


# ---- the twins, word for word --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ref.SIZES)
@pytest.mark.parametrize("P", COUNTS)
def test_accumulate_planes_equals_per_plane_twin(P, W, H):
    s = plane_set(W, H)
    kw = dict(max_history=32, depth_tol=TOL, normal_cos=NCOS)
    out, hist = rt.host_ao_accumulate_planes(W, H, s["cur"][:P], s["motion"], s["gc"], s["prev"][:P], s["hist_prev"],
                                             s["gp"], **kw)
    first, hist1 = rt.host_ao_accumulate_planes(W, H, s["cur"][:P], s["motion"], s["gc"], **kw)
    inpl, hist2 = rt.host_ao_accumulate_planes(W, H, s["cur"][:P], s["motion"], s["gc"], s["prev"][:P], s["hist_prev"],
                                               s["gp"], in_place=True, **kw)
    assert out.shape == (P, W * H) and hist.shape == (W * H,)
    for p in range(P):
        ao, h = rt.host_ao_accumulate(W, H, s["cur"][p], s["motion"], s["gc"], s["prev"][p], s["hist_prev"], s["gp"],
                                      **kw)
        same(out[p], ao, f"out[{p}]")
        same(hist, h, f"hist_out against plane {p}'s")
        same(inpl[p], ao, f"in place out[{p}]")
        ao1, h1 = rt.host_ao_accumulate(W, H, s["cur"][p], s["motion"], s["gc"], **kw)
        same(first[p], ao1, f"first frame out[{p}]")
        same(hist1, h1, "first frame hist_out")
    same(hist2, hist, "in place hist_out")


@pytest.mark.parametrize("W,H", ref.SIZES)
@pytest.mark.parametrize("P", COUNTS)
def test_atrous_planes_equals_per_plane_twin(P, W, H):
    s = plane_set(W, H)
    for it in range(1, 6):
        out = rt.host_ao_atrous_planes(W, H, s["prev"][:P], s["gc"], iterations=it, depth_tol=TOL, normal_cos=NCOS)
        assert out.shape == (P, W * H)
        for p in range(P):
            want = rt.host_ao_atrous(W, H, s["prev"][p], s["gc"], iterations=it, depth_tol=TOL, normal_cos=NCOS)
            same(out[p], want, f"{it} iterations, out[{p}]")


def test_step_16_taps_inside_and_outside_at_70_x_67():
    """70 x 67 is the smallest size of the list at which a step-16 tap (+-32 px) is in the frame for some pixels and
    outside for others, in both directions: what the fifth iteration's mask has to tell apart."""
    W, H = 70, 67
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    for c, n in ((x, W), (y, H)):
        assert np.any((c - 32 >= 0) & (c + 32 < n)) and np.any(c - 32 < 0) and np.any(c + 32 >= n)
    assert all(w < 65 or h < 65 for w, h in ref.SIZES[:-1])


def test_three_chained_frames():
    """Each frame's outputs are the next frame's history, batched and per plane: the shared history plane and the
    planes stay equal, and so does what is shown (3 a-trous iterations)."""
    W, H, P = 37, 21, 7
    s = plane_set(W, H)
    b_out = b_hist = None
    per = [(None, None)] * P
    for f in range(3):
        cur = np.stack([ref.synthetic(W, H, seed=p + 17 * f)["ao_cur"] for p in range(P)])
        gprev = None if f == 0 else s["gc"].copy()  # a plane of its own: no two pointers of a call may be equal
        b_out, b_hist = rt.host_ao_accumulate_planes(W, H, cur, s["motion"], s["gc"], b_out, b_hist, gprev)
        shown = rt.host_ao_atrous_planes(W, H, b_out, s["gc"], iterations=3)
        for p in range(P):
            per[p] = rt.host_ao_accumulate(W, H, cur[p], s["motion"], s["gc"], per[p][0], per[p][1], gprev)
            same(b_out[p], per[p][0], f"frame {f} out[{p}]")
            same(b_hist, per[p][1], f"frame {f} hist_out")
            same(shown[p], rt.host_ao_atrous(W, H, per[p][0], s["gc"], iterations=3), f"frame {f} shown[{p}]")
    assert b_hist.max() > 2.0  # the history did chain


# ---- a skipped tap is skipped, not multiplied by zero; planes do not leak into each other -----------------------------
def test_nan_behind_skipped_taps_stays_out():
    W, H, P = 37, 21, 3
    s = plane_set(W, H)
    surface = s["gc"][:, 3] != 0
    # a-trous: NaN in plane 1 wherever the guide has no surface (those taps are skipped by every surface pixel)
    clean = np.array(s["prev"][:P])
    dirty = clean.copy()
    dirty[1, ~surface] = np.nan
    assert np.isnan(dirty[1]).sum() > 20
    for it in range(1, 6):
        got = rt.host_ao_atrous_planes(W, H, dirty, s["gc"], iterations=it)
        base = rt.host_ao_atrous_planes(W, H, clean, s["gc"], iterations=it)
        want1 = rt.host_ao_atrous(W, H, dirty[1], s["gc"], iterations=it)
        assert not np.isnan(got[1, surface]).any(), f"{it} iterations: a skipped tap's NaN reached a surface pixel"
        same(got[1, surface], want1[surface], f"{it} iterations: plane 1 on the surface pixels")
        same(got[0], base[0], f"{it} iterations: plane 0 changed with plane 1's content")
        same(got[2], base[2], f"{it} iterations: plane 2 changed with plane 1's content")
    # accumulate: NaN in prev[1] wherever the previous guide has no surface (those taps are never accepted)
    gone = s["gp"][:, 3] == 0
    pclean = np.array(s["prev"][:P])
    pdirty = pclean.copy()
    pdirty[1, gone] = np.nan
    args = (W, H, s["cur"][:P], s["motion"], s["gc"])
    got, hist = rt.host_ao_accumulate_planes(*args, pdirty, s["hist_prev"], s["gp"])
    base, hist0 = rt.host_ao_accumulate_planes(*args, pclean, s["hist_prev"], s["gp"])
    want1, _ = rt.host_ao_accumulate(W, H, s["cur"][1], s["motion"], s["gc"], pdirty[1], s["hist_prev"], s["gp"])
    assert not np.isnan(got[1]).any()
    same(got[1], want1, "accumulate: plane 1")
    same(got[0], base[0], "accumulate: plane 0 changed with plane 1's content")
    same(got[2], base[2], "accumulate: plane 2 changed with plane 1's content")
    same(hist, hist0, "accumulate: the history changed with plane 1's content")


# ---- every refused call ------------------------------------------------------------------------------------------------
SENTINEL = F(-7.0)


class Raw:
    """The C entry points on hand-made tables: P planes of n floats per table, outputs pre-filled with a sentinel."""

    def __init__(self, W=9, H=5, P=3):
        self.W, self.H, self.P, n = W, H, P, W * H
        self.n = n
        mk = lambda k: np.zeros((k, n), F)  # noqa: E731
        self.cur, self.prev, self.src = mk(P), mk(P), mk(P)
        self.out, self.tmp = np.full((P, n), SENTINEL, F), np.full((P, n), SENTINEL, F)
        self.hist_out = np.full(n, SENTINEL, F)
        self.hist_prev = np.zeros(n, F)
        self.motion, self.gc, self.gp = (np.zeros((n, 4), F) for _ in range(3))

    @staticmethod
    def rows(a):
        return [a.ctypes.data + r * a.strides[0] for r in range(a.shape[0])]

    @staticmethod
    def table(ptrs):
        return None if ptrs is None else (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)

    def accumulate(self, W=None, H=None, params=(32, 0.02, 0.9), nplanes=None, **kw):
        a = dict(cur=self.rows(self.cur), prev=self.rows(self.prev), out=self.rows(self.out),
                 motion=self.motion.ctypes.data, guide_cur=self.gc.ctypes.data, guide_prev=self.gp.ctypes.data,
                 hist_prev=self.hist_prev.ctypes.data, hist_out=self.hist_out.ctypes.data)
        a.update(kw)
        p = None if params is None else ctypes.byref(rt.rt_ao_temporal_params(*params))
        return rt.lib.rt_host_ao_accumulate_planes(
            self.W if W is None else W, self.H if H is None else H, p, self.P if nplanes is None else nplanes,
            self.table(a["cur"]), a["motion"], a["guide_cur"], self.table(a["prev"]), a["hist_prev"], a["guide_prev"],
            self.table(a["out"]), a["hist_out"])

    def atrous(self, W=None, H=None, params=(3, 0.02, 0.9), nplanes=None, **kw):
        a = dict(src=self.rows(self.src), out=self.rows(self.out), tmp=self.rows(self.tmp), guide=self.gc.ctypes.data)
        a.update(kw)
        p = None if params is None else ctypes.byref(rt.rt_ao_atrous_params(*params))
        return rt.lib.rt_host_ao_atrous_planes(
            self.W if W is None else W, self.H if H is None else H, p, self.P if nplanes is None else nplanes,
            self.table(a["src"]), a["guide"], self.table(a["out"]), self.table(a["tmp"]))

    def untouched(self):
        return all(bool((a == SENTINEL).all()) for a in (self.out, self.tmp, self.hist_out))


def refused(st, status=None, *names):
    assert st == (rt.RT_E_INVALID if status is None else status), rt.lib.rt_status_string(st)
    msg = rt.lib.rt_host_last_error().decode()
    assert len(msg) > 20, msg
    for name in names:
        assert name in msg, f"{msg!r} does not name {name}"
    return msg


def swap(ptrs, i, value):
    return ptrs[:i] + [value] + ptrs[i + 1:]


def test_accumulate_planes_refusals_write_nothing():
    r = Raw()
    cur, prev, out = r.rows(r.cur), r.rows(r.prev), r.rows(r.out)
    many = np.zeros((18, r.n), F)
    refused(r.accumulate(nplanes=0), None, "nplanes")
    refused(r.accumulate(nplanes=18, cur=r.rows(many), prev=r.rows(many.copy()), out=r.rows(many.copy())), None,
            "nplanes", "17")
    # a NULL table, a NULL entry
    refused(r.accumulate(cur=None), None, "cur")
    refused(r.accumulate(out=None), None, "out")
    refused(r.accumulate(cur=swap(cur, 2, None)), None, "cur[2]")
    refused(r.accumulate(out=swap(out, 1, None)), None, "out[1]")
    refused(r.accumulate(prev=swap(prev, 0, None)), None, "prev[0]")
    # a misaligned plane
    refused(r.accumulate(cur=swap(cur, 1, cur[1] + 2)), None, "cur[1]")
    refused(r.accumulate(out=swap(out, 2, out[2] + 1)), None, "out[2]")
    refused(r.accumulate(prev=swap(prev, 2, prev[2] + 2)), None, "prev[2]")
    refused(r.accumulate(motion=r.motion.ctypes.data + 2), None, "motion")
    refused(r.accumulate(hist_out=r.hist_out.ctypes.data + 2), None, "hist_out")
    # any two pointers equal, other than out[p] == cur[p]
    refused(r.accumulate(out=swap(out, 1, out[0])), None, "out[0]", "out[1]")
    refused(r.accumulate(cur=swap(cur, 2, cur[0])), None, "cur[0]", "cur[2]")
    refused(r.accumulate(out=swap(out, 1, cur[0])), None, "out[1]", "cur[0]")
    refused(r.accumulate(out=swap(out, 0, prev[0])), None, "out[0]", "prev[0]")
    refused(r.accumulate(out=swap(out, 2, prev[1])), None, "out[2]", "prev[1]")
    refused(r.accumulate(prev=swap(prev, 1, cur[1])), None, "prev[1]", "cur[1]")
    refused(r.accumulate(prev=swap(prev, 1, prev[2])), None, "prev[1]", "prev[2]")
    refused(r.accumulate(hist_out=cur[2]), None, "hist_out", "cur[2]")
    refused(r.accumulate(hist_out=out[0]), None, "hist_out", "out[0]")
    refused(r.accumulate(out=swap(out, 1, r.motion.ctypes.data)), None, "out[1]", "motion")
    refused(r.accumulate(out=swap(out, 1, r.gc.ctypes.data)), None, "out[1]", "guide_cur")
    refused(r.accumulate(out=swap(out, 1, r.gp.ctypes.data)), None, "out[1]", "guide_prev")
    refused(r.accumulate(out=swap(out, 1, r.hist_prev.ctypes.data)), None, "out[1]", "hist_prev")
    refused(r.accumulate(hist_out=r.hist_prev.ctypes.data), None, "hist_out", "hist_prev")
    refused(r.accumulate(guide_prev=r.gc.ctypes.data), None, "guide_prev", "guide_cur")
    refused(r.accumulate(cur=swap(cur, 0, r.motion.ctypes.data)), None, "cur[0]", "motion")
    # only some of the prev arguments
    refused(r.accumulate(prev=None), None, "prev")
    refused(r.accumulate(hist_prev=None), None, "prev")
    refused(r.accumulate(guide_prev=None), None, "prev")
    refused(r.accumulate(prev=None, guide_prev=None), None, "prev")
    # rt_ao_accumulate's own cases
    for params in ((0, 0.02, 0.9), (1025, 0.02, 0.9), (32, 0.0, 0.9), (32, float("inf"), 0.9), (32, float("nan"), 0.9),
                   (32, 0.02, 1.0), (32, 0.02, -1.5), (32, 0.02, float("nan")), None):
        refused(r.accumulate(params=params))
    refused(r.accumulate(motion=None), None, "motion")
    refused(r.accumulate(guide_cur=None), None, "guide_cur")
    refused(r.accumulate(hist_out=None), None, "hist_out")
    refused(r.accumulate(W=0))
    refused(r.accumulate(H=0))
    refused(r.accumulate(W=1 << 16, H=1 << 15), rt.RT_E_UNSUPPORTED)
    refused(r.accumulate(W=(1 << 30) + 1, H=1), rt.RT_E_UNSUPPORTED)
    assert r.untouched()
    # what is allowed: the in-place form, and the first frame
    assert r.accumulate(out=cur) == rt.RT_OK
    assert r.accumulate(prev=None, hist_prev=None, guide_prev=None) == rt.RT_OK
    assert not (r.out == SENTINEL).any() and not (r.hist_out == SENTINEL).any() and (r.tmp == SENTINEL).all()


def test_atrous_planes_refusals_write_nothing():
    r = Raw()
    src, out, tmp = r.rows(r.src), r.rows(r.out), r.rows(r.tmp)
    many = np.zeros((18, r.n), F)
    refused(r.atrous(nplanes=0), None, "nplanes")
    refused(r.atrous(nplanes=18, src=r.rows(many), out=r.rows(many.copy()), tmp=r.rows(many.copy())), None,
            "nplanes", "17")
    refused(r.atrous(src=None), None, "in")
    refused(r.atrous(out=None), None, "out")
    refused(r.atrous(tmp=None), None, "tmp")  # 3 iterations
    refused(r.atrous(params=(2, 0.02, 0.9), tmp=None), None, "tmp")
    refused(r.atrous(src=swap(src, 1, None)), None, "in[1]")
    refused(r.atrous(out=swap(out, 0, None)), None, "out[0]")
    refused(r.atrous(tmp=swap(tmp, 2, None)), None, "tmp[2]")
    refused(r.atrous(params=(1, 0.02, 0.9), tmp=swap(tmp, 2, None)), None, "tmp[2]")  # a table that is given is whole
    refused(r.atrous(src=swap(src, 1, src[1] + 2)), None, "in[1]")
    refused(r.atrous(out=swap(out, 2, out[2] + 1)), None, "out[2]")
    refused(r.atrous(tmp=swap(tmp, 0, tmp[0] + 2)), None, "tmp[0]")
    refused(r.atrous(guide=r.gc.ctypes.data + 2), None, "guide")
    refused(r.atrous(out=swap(out, 0, src[0])), None, "out[0]", "in[0]")
    refused(r.atrous(out=swap(out, 1, src[2])), None, "out[1]", "in[2]")
    refused(r.atrous(src=swap(src, 1, src[0])), None, "in[0]", "in[1]")
    refused(r.atrous(out=swap(out, 2, out[1])), None, "out[1]", "out[2]")
    refused(r.atrous(tmp=swap(tmp, 0, out[1])), None, "tmp[0]", "out[1]")
    refused(r.atrous(tmp=swap(tmp, 0, out[0])), None, "tmp[0]", "out[0]")
    refused(r.atrous(tmp=swap(tmp, 1, src[0])), None, "tmp[1]", "in[0]")
    refused(r.atrous(tmp=swap(tmp, 1, tmp[2])), None, "tmp[1]", "tmp[2]")
    refused(r.atrous(out=swap(out, 0, r.gc.ctypes.data)), None, "out[0]", "guide")
    refused(r.atrous(src=swap(src, 2, r.gc.ctypes.data)), None, "in[2]", "guide")
    refused(r.atrous(tmp=swap(tmp, 2, r.gc.ctypes.data)), None, "tmp[2]", "guide")
    for params in ((0, 0.02, 0.9), (6, 0.02, 0.9), (3, 0.0, 0.9), (3, float("nan"), 0.9), (3, float("inf"), 0.9),
                   (3, 0.02, 1.0), (3, 0.02, float("nan")), None):
        refused(r.atrous(params=params))
    refused(r.atrous(guide=None), None, "guide")
    refused(r.atrous(W=0))
    refused(r.atrous(H=0))
    refused(r.atrous(W=1 << 16, H=1 << 15), rt.RT_E_UNSUPPORTED)
    assert r.untouched()
    # one iteration: tmp may be NULL, and a tmp that is given stays unwritten
    assert r.atrous(params=(1, 0.02, 0.9), tmp=None) == rt.RT_OK
    assert r.atrous(params=(1, 0.02, 0.9)) == rt.RT_OK
    assert not (r.out == SENTINEL).any() and (r.tmp == SENTINEL).all()
    assert r.atrous(params=(2, 0.02, 0.9)) == rt.RT_OK
    assert not (r.tmp == SENTINEL).any()


def test_python_wrappers_check_the_plane_sets():
    W, H = 3, 2
    s = plane_set(W, H)
    with pytest.raises(ValueError):
        rt.host_ao_accumulate_planes(W, H, s["cur"][:2], s["motion"], s["gc"], s["prev"][:3], s["hist_prev"], s["gp"])
    with pytest.raises(ValueError):
        rt.host_ao_atrous_planes(W, H, [s["prev"][0][:-1]], s["gc"])
    with pytest.raises(rt.RtError) as e:
        rt.host_ao_atrous_planes(W, H, s["prev"][:2], s["gc"], iterations=6)
    assert e.value.status == rt.RT_E_INVALID and "iterations" in str(e.value)
    assert rt.RT_MAX_FILTER_PLANES == 17
