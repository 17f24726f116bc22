"""The AO filter's host twins (rt_host_denoise_guide, rt_host_ao_accumulate, rt_host_ao_atrous) without a GPU: bit
equality with the numpy restatement of tests/denoise_reference.py on synthetic planes, the exact semantics of a static
frame, no bleeding across depth and normal edges, pass-through of invalid pixels, footprints, and every refused
argument. Tolerance 0 except where a bound is derived in the test."""
import ctypes

import numpy as np
import pytest

import realtimeraytracing_gradproject_amd as rt

import denoise_reference as ref

F = np.float32
TOL, NCOS = ref.DEPTH_TOL, ref.NORMAL_COS


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def guides(syn):
    """(guide_cur, guide_prev) of a synthetic set through the host twin (cur from motion's w_cur with stride 4)."""
    return (rt.host_denoise_guide(syn["normal_cur"], syn["motion"][:, 3]),
            rt.host_denoise_guide(syn["normal_prev"], syn["depth_prev"]))


@pytest.mark.parametrize("W,H", ref.SIZES)
def test_guide_equals_restatement(W, H):
    syn = ref.synthetic(W, H)
    gc, gp = guides(syn)
    assert np.array_equal(bits(gc), bits(ref.guide(syn["normal_cur"], syn["motion"][:, 3])))
    assert np.array_equal(bits(gp), bits(ref.guide(syn["normal_prev"], syn["depth_prev"])))
    live = gc[:, 3] != 0
    assert np.all(gc[~live] == 0)
    assert np.all(np.abs(np.linalg.norm(gc[live, :3].astype(np.float64), axis=1) - 1.0) < 1e-6)
    if W * H >= 100:
        assert 0.05 < 1.0 - live.mean() < 0.2  # about a tenth of the pixels is invalid, in every way
        n3 = syn["normal_cur"][:, :3].astype(np.float64)
        assert np.any(np.abs(np.linalg.norm(n3[live], axis=1) - 1.0) > 0.5)  # non-unit normals are there


@pytest.mark.parametrize("W,H", ref.SIZES)
def test_accumulate_equals_restatement(W, H):
    syn = ref.synthetic(W, H)
    gc, gp = guides(syn)
    args = (W, H, syn["ao_cur"], syn["motion"], gc, syn["ao_prev"], syn["hist_prev"], gp)
    ao_r, hist_r, taps, acc = ref.accumulate(*args, max_history=32, depth_tol=TOL, normal_cos=NCOS)
    if W * H >= 100:  # the planes reach every branch: each class holds a tenth of the valid pixels
        valid, full, some, none = ref.classes(gc, taps, acc)
        print(f"{W}x{H}: valid {valid}, all taps accepted {full}, some {some}, none {none}")
        assert min(full, some, none) >= 0.10 * valid, (valid, full, some, none)
        assert np.any(taps < 4) and np.any(~np.isfinite(syn["motion"][:, 0]))
    ao, hist = rt.host_ao_accumulate(*args, max_history=32, depth_tol=TOL, normal_cos=NCOS)
    assert np.array_equal(bits(ao), bits(ao_r))
    assert np.array_equal(bits(hist), bits(hist_r))
    # the first frame: no history is sought
    ao, hist = rt.host_ao_accumulate(W, H, syn["ao_cur"], syn["motion"], gc)
    assert np.array_equal(bits(ao), bits(syn["ao_cur"]))
    assert np.array_equal(hist, (gc[:, 3] != 0).astype(F))
    ao_r, hist_r, _, _ = ref.accumulate(W, H, syn["ao_cur"], syn["motion"], gc)
    assert np.array_equal(bits(ao), bits(ao_r)) and np.array_equal(bits(hist), bits(hist_r))


@pytest.mark.parametrize("W,H", ref.SIZES)
def test_atrous_equals_restatement(W, H):
    syn = ref.synthetic(W, H)
    gc, _ = guides(syn)
    for it in range(1, 6):
        got = rt.host_ao_atrous(W, H, syn["ao_prev"], gc, iterations=it, depth_tol=TOL, normal_cos=NCOS)
        want = ref.atrous(W, H, syn["ao_prev"], gc, it, TOL, NCOS)
        assert np.array_equal(bits(got), bits(want)), f"{it} iterations"
    if W * H >= 100:  # the edge weights take every kind of value
        live = gc[:, 3] != 0
        one = ref.atrous(W, H, syn["ao_prev"], gc, 1, TOL, NCOS)
        assert np.any(one[live] != syn["ao_prev"][live])


def flat_guide(W, H, normal=(0.0, 0.0, 1.0), depth=5.0):
    g = np.zeros((W * H, 4), F)
    g[:, :3] = normal
    g[:, 3] = depth
    return g


def test_static_frame_counts_history_and_keeps_a_constant_input():
    W, H, n = 9, 7, 63
    g = flat_guide(W, H)
    g[5] = 0.0  # no surface: history 0 throughout
    motion = np.zeros((n, 4), F)
    motion[:, 2:] = 5.0
    rng = np.random.default_rng(3)
    v = rng.random(n).astype(F)
    ao, hist = rt.host_ao_accumulate(W, H, v, motion, g, max_history=6)
    for frame in range(2, 10):
        ao2, hist = rt.host_ao_accumulate(W, H, v, motion, g, ao, hist, g, max_history=6)
        want = np.full(n, min(frame, 6), F)
        want[5] = 0.0
        assert np.array_equal(hist, want)
        # an unchanged input: a = (1 * v) / 1 (the zero-weight taps are skipped), v + (1 / n) * (v - v) = v
        assert np.array_equal(bits(ao2), bits(ao))
        ao = ao2
    # max_history = 1 returns ao_cur whatever the history holds
    cur = rng.random(n).astype(F)
    ao3, hist3 = rt.host_ao_accumulate(W, H, cur, motion, g, ao, hist, g, max_history=1)
    assert np.array_equal(bits(ao3), bits(cur))
    want = np.ones(n, F)
    want[5] = 0.0
    assert np.array_equal(hist3, want)


def test_static_mean_of_frames():
    """With zero motion the accumulated value is the running mean: frame k blends 1 / k."""
    W, H, n = 5, 4, 20
    g = flat_guide(W, H)
    motion = np.zeros((n, 4), F)
    motion[:, 2:] = 5.0
    rng = np.random.default_rng(4)
    frames = (rng.random((16, n)) < 0.5).astype(F)
    ao, hist = rt.host_ao_accumulate(W, H, frames[0], motion, g)
    for k in range(1, 16):
        ao, hist = rt.host_ao_accumulate(W, H, frames[k], motion, g, ao, hist, g)
    assert np.all(hist == 16)
    assert np.abs(ao.astype(np.float64) - frames.astype(np.float64).mean(axis=0)).max() <= 1e-5


@pytest.mark.parametrize("edge", ["depth", "normal"])
def test_no_bleeding_across_an_edge(edge):
    """Two regions, each with a constant AO, separated by more than the filter accepts at any step: depths 1 and 10
    (|dz| = 9 against (0.02 * 10) * 16 = 3.2 at the widest) or perpendicular normals (dot 0 < normal_cos). Every
    cross-region weight is then exactly 0 and a pixel's value is sum(w c) / sum(w): 25 products, 25 additions and one
    quotient, each within 2^-24 relative, so within 27 ulp of the constant per iteration."""
    W, H = 70, 67
    yy, xx = np.divmod(np.arange(W * H), W)
    left = xx + yy // 3 < 40  # a slanted edge: both lattices see it
    g = flat_guide(W, H)
    if edge == "depth":
        g[:, 3] = np.where(left, 1.0, 10.0)
    else:
        g[~left, :3] = (1.0, 0.0, 0.0)
    c = np.where(left, F(0.3), F(0.7)).astype(F)
    for it in range(1, 6):
        out = rt.host_ao_atrous(W, H, c, g, iterations=it, depth_tol=0.02, normal_cos=0.9)
        ulps = np.abs(out.astype(np.float64) - c.astype(np.float64)) / np.spacing(c).astype(np.float64)
        print(f"{edge} edge, {it} iterations: {ulps.max()} ulp")
        assert ulps.max() <= 27 * it


def test_invalid_pixels_pass_through():
    W, H = 37, 21
    syn = ref.synthetic(W, H)
    gc, gp = guides(syn)
    dead = gc[:, 3] == 0
    assert dead.any()
    ao, hist = rt.host_ao_accumulate(W, H, syn["ao_cur"], syn["motion"], gc, syn["ao_prev"], syn["hist_prev"], gp)
    assert np.array_equal(bits(ao[dead]), bits(syn["ao_cur"][dead])) and np.all(hist[dead] == 0)
    marked = syn["ao_prev"].copy()
    marked[dead] = np.linspace(2.0, 3.0, int(dead.sum()), dtype=F)
    for it in (1, 2, 5):
        out = rt.host_ao_atrous(W, H, marked, gc, iterations=it)
        assert np.array_equal(bits(out[dead]), bits(marked[dead]))
    # ... and an invalid pixel's value reaches no valid pixel (it is skipped as a tap)
    assert np.array_equal(bits(rt.host_ao_atrous(W, H, marked, gc, iterations=5)[~dead]),
                          bits(rt.host_ao_atrous(W, H, syn["ao_prev"], gc, iterations=5)[~dead]))


def test_footprints():
    W, H = 70, 67
    n = W * H
    yy, xx = np.divmod(np.arange(n), W)
    g = flat_guide(W, H)
    rng = np.random.default_rng(5)
    v = rng.random(n).astype(F)
    px, py = 33, 30
    poked = v.copy()
    poked[py * W + px] += F(64.0)
    # iterations 1..3: the footprint is the sum of the steps' 5 x 5 lattices, every pixel within radius 2, 6, 14
    for it, radius in ((1, 2), (2, 6), (3, 14)):
        a = rt.host_ao_atrous(W, H, v, g, iterations=it)
        b = rt.host_ao_atrous(W, H, poked, g, iterations=it)
        changed = bits(a) != bits(b)
        inside = (np.abs(xx - px) <= radius) & (np.abs(yy - py) <= radius)
        assert not changed[~inside].any()
        assert changed[inside].all()  # a flat guide: every weight in the footprint is positive
    # the accumulate pass reads the 2 x 2 taps at the reprojected position, nothing else of the previous frame
    motion = np.zeros((n, 4), F)
    motion[:, 0], motion[:, 1], motion[:, 2:] = 1.25, -2.5, 5.0
    hist = np.full(n, 3.0, F)
    a, _ = rt.host_ao_accumulate(W, H, v, motion, g, v, hist, g)
    b, _ = rt.host_ao_accumulate(W, H, v, motion, g, poked, hist, g)
    changed = bits(a) != bits(b)
    # pixel (x, y) reads (x + 1, x + 2) x (y - 3, y - 2): the poke at (33, 30) is seen from x in {31, 32}, y in {32, 33}
    want = np.isin(xx, (px - 2, px - 1)) & np.isin(yy, (py + 2, py + 3))
    assert np.array_equal(changed, want)
    # ... and only its own pixel of the current frame
    b, _ = rt.host_ao_accumulate(W, H, poked, motion, g, v, hist, g)
    assert np.array_equal(bits(a) != bits(b), (xx == px) & (yy == py))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_refused_arguments_write_nothing():
    W, H, n = 6, 5, 30
    g, gp = flat_guide(W, H), flat_guide(W, H)
    motion = np.zeros((n, 4), F)
    motion[:, 2:] = 5.0
    cur, prev, hist = np.full(n, 0.5, F), np.full(n, 0.25, F), np.full(n, 2.0, F)
    out, hout, tmp = np.full(n, -1.0, F), np.full(n, -1.0, F), np.full(n, -1.0, F)
    nrm, depth, gout = np.ones((n, 4), F), np.ones(n, F), np.full((n, 4), -1.0, F)
    INV = rt.RT_E_INVALID

    # guide
    L = rt.lib
    assert L.rt_host_denoise_guide(n, _p(nrm), _p(depth), 1, _p(gout)) == rt.RT_OK
    gout[:] = -1.0
    assert L.rt_host_denoise_guide(n, None, _p(depth), 1, _p(gout)) == INV
    assert L.rt_host_denoise_guide(n, _p(nrm), None, 1, _p(gout)) == INV
    assert L.rt_host_denoise_guide(n, _p(nrm), _p(depth), 1, None) == INV
    assert L.rt_host_denoise_guide(n, _p(nrm), _p(depth), 0, _p(gout)) == INV
    assert L.rt_host_denoise_guide(n, _p(gout), _p(depth), 1, _p(gout)) == INV  # in place
    assert L.rt_host_denoise_guide(n, _p(nrm), ctypes.c_void_p(gout.ctypes.data + 12), 4, _p(gout)) == INV
    assert L.rt_host_denoise_guide(0, None, None, 1, None) == rt.RT_OK
    assert L.rt_host_denoise_guide(1 << 31, _p(nrm), _p(depth), 1, _p(gout)) == rt.RT_E_UNSUPPORTED  # as W x H
    assert L.rt_host_denoise_guide(0xFFFFFFFF, _p(nrm), _p(depth), 1, _p(gout)) == rt.RT_E_UNSUPPORTED
    assert np.all(gout == -1.0)

    # accumulate
    def acc(params=(32, 0.02, 0.9), w=W, h=H, **kw):
        a = dict(ao_cur=cur, motion=motion, guide_cur=g, ao_prev=prev, hist_prev=hist, guide_prev=gp, ao_out=out,
                 hist_out=hout)
        a.update(kw)
        p = None if params is None else ctypes.byref(rt.rt_ao_temporal_params(*params))
        return L.rt_host_ao_accumulate(w, h, p, *(_p(a[k]) for k in ("ao_cur", "motion", "guide_cur", "ao_prev",
                                                                     "hist_prev", "guide_prev", "ao_out", "hist_out")))

    bad_params = [None, (0, 0.02, 0.9), (1025, 0.02, 0.9), (32, 0.0, 0.9), (32, -1.0, 0.9), (32, np.inf, 0.9),
                  (32, np.nan, 0.9), (32, 0.02, 1.0), (32, 0.02, -1.5), (32, 0.02, np.nan)]
    for p in bad_params:
        assert acc(params=p) == INV, p
    assert acc(w=0) == INV and acc(h=0) == INV
    assert acc(w=1 << 16, h=1 << 15) == rt.RT_E_UNSUPPORTED
    for k in ("ao_cur", "motion", "guide_cur", "ao_out", "hist_out", "ao_prev", "hist_prev", "guide_prev"):
        assert acc(**{k: None}) == INV, k  # a prev plane alone missing: only some of the three
    assert acc(ao_prev=None, hist_prev=None) == INV
    for o in ("ao_out", "hist_out"):
        for k in ("ao_prev", "hist_prev", "guide_prev", "motion", "guide_cur"):
            big = np.full((n, 4), -1.0, F)  # large enough to stand for either
            assert acc(**{o: big, k: big}) == INV, (o, k)
            assert np.all(big == -1.0)
    assert acc(hist_out=out) == INV
    assert acc(hist_out=cur) == INV
    assert np.all(out == -1.0) and np.all(hout == -1.0) and np.all(cur == 0.5)
    assert acc(params=(32, 0.02, -1.0)) == rt.RT_OK  # the bounds themselves are accepted
    inplace = cur.copy()
    assert acc(ao_cur=inplace, ao_out=inplace) == rt.RT_OK  # in place over ao_cur
    assert np.array_equal(bits(inplace), bits(out))
    assert acc(ao_prev=None, hist_prev=None, guide_prev=None) == rt.RT_OK

    # a-trous
    out[:] = -1.0

    def atr(params=(3, 0.02, 0.9), w=W, h=H, **kw):
        a = dict(ao_in=cur, guide=g, ao_out=out, tmp=tmp)
        a.update(kw)
        p = None if params is None else ctypes.byref(rt.rt_ao_atrous_params(*params))
        return L.rt_host_ao_atrous(w, h, p, *(_p(a[k]) for k in ("ao_in", "guide", "ao_out", "tmp")))

    for p in [None, (0, 0.02, 0.9), (6, 0.02, 0.9), (3, 0.0, 0.9), (3, np.inf, 0.9), (3, np.nan, 0.9), (3, 0.02, 1.0),
              (3, 0.02, -1.01), (3, 0.02, np.nan)]:
        assert atr(params=p) == INV, p
    assert atr(w=0) == INV and atr(h=0) == INV
    assert atr(w=1 << 16, h=1 << 15) == rt.RT_E_UNSUPPORTED
    for k in ("ao_in", "guide", "ao_out", "tmp"):
        assert atr(**{k: None}) == INV, k
    big = np.full((n, 4), -1.0, F)
    for a, b in (("ao_in", "guide"), ("ao_in", "ao_out"), ("ao_in", "tmp"), ("guide", "ao_out"), ("guide", "tmp"),
                 ("ao_out", "tmp")):
        assert atr(**{a: big, b: big}) == INV, (a, b)
    assert np.all(big == -1.0) and np.all(out == -1.0) and np.all(tmp == -1.0)
    assert atr(params=(1, 0.02, 0.9), tmp=None) == rt.RT_OK  # one iteration needs no tmp
    assert np.all(out != -1.0) and np.all(tmp == -1.0) and np.all(cur == 0.5)  # ... and ao_in is never written
    first = out.copy()
    assert atr(params=(1, 0.02, 0.9)) == rt.RT_OK
    assert np.array_equal(bits(first), bits(out)) and np.all(tmp == -1.0)  # one iteration does not touch tmp
    for it in (2, 3, 4, 5):  # the last iteration lands in ao_out whatever the parity
        assert atr(params=(it, 0.02, 0.9)) == rt.RT_OK
        assert np.array_equal(bits(out), bits(rt.host_ao_atrous(W, H, cur, g, iterations=it)))


def test_python_wrappers_refuse_what_the_library_refuses():
    g = flat_guide(3, 2)
    with pytest.raises(rt.RtError):
        rt.host_ao_atrous(3, 2, np.zeros(6, F), g, iterations=6)
    with pytest.raises(rt.RtError):
        rt.host_ao_accumulate(3, 2, np.zeros(6, F), np.zeros((6, 4), F), g, max_history=0)
    with pytest.raises(ValueError):
        rt.host_ao_atrous(3, 2, np.zeros(5, F), g)
    with pytest.raises(ValueError):
        rt.host_denoise_guide(np.zeros((6, 4), F), np.zeros(5, F))
