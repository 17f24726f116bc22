"""The packet triangle leaf leaves a test early when no lane can accept (rt_trace.hip packet_tri, RT_TRI_EXIT): after
u it exits when no owning lane has 0 <= u <= 1, after v when none has v >= 0 and u + v <= 1. Both are sound only if
the shipped acceptance (rt_device.hpp moller_trumbore_flat: min(u, v) >= 0 and u + v <= 1) implies them for every pair
of float32 values, NaN and +-0 included. Checked here in numpy float32 (np.fmin is C's fminf, as v_min_f32) over the
special values of tests/test_acceptance.py and over random pairs around the triangle's edges."""
import numpy as np

from test_acceptance import _specials


def _shipped(u, v):
    return (np.fmin(u, v) >= 0) & ((u + v) <= 1)


def _first_exit_keeps(u):
    """the lanes the exit after u counts as candidates"""
    return (u >= 0) & (u <= 1)


def _second_exit_keeps(u, v):
    return (v >= 0) & ((u + v) <= 1)


def _check(u, v):
    with np.errstate(invalid="ignore", over="ignore"):
        ok = _shipped(u, v)
        assert np.all(_first_exit_keeps(u)[ok]), "an accepting lane outside 0 <= u <= 1"
        assert np.all(_second_exit_keeps(u, v)[ok]), "an accepting lane outside v >= 0, u + v <= 1"
    return int(ok.sum())


def test_exit_conditions_hold_on_special_values():
    s = _specials()
    u, v = np.meshgrid(s, s)
    assert _check(u, v) > 0


def test_exit_conditions_hold_near_the_edges():
    rng = np.random.default_rng(0xE817)
    n = 2_000_000
    # as test_acceptance: u over the range and a little beyond, v on the u + v = 1 edge a few ulps either way, and w
    # around 0; every pairing of them, so each edge and each corner is approached from both sides
    u = rng.uniform(-0.01, 1.01, n).astype(np.float32)
    v = (np.float32(1) - u).astype(np.float32)
    v = (v.view(np.int32) + rng.integers(-3, 4, n).astype(np.int32)).view(np.float32)
    w = rng.uniform(-1e-6, 1e-6, n).astype(np.float32)
    # u = 1 and v = 0 a few ulps either way (the vertex the u <= 1 bound guards)
    one = (np.full(n, 1, np.float32).view(np.int32) + rng.integers(-3, 4, n).astype(np.int32)).view(np.float32)
    accepted = 0
    for a, b in ((u, v), (v, u), (u, w), (w, u), (w, w), (one, w), (w, one)):
        accepted += _check(a, b)
    assert accepted > n  # the pairs do straddle the acceptance


def test_a_wave_without_candidates_has_no_accepting_lane():
    """The exit as the leaf takes it: 64 lanes of which a few own the triangle, exit when no owning lane is a
    candidate. No wave that exits holds an owning lane that accepts."""
    rng = np.random.default_rng(7)
    shape = (50_000, 64)
    u = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    v = rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    u[rng.random(shape) < 0.02] = np.nan
    v[rng.random(shape) < 0.02] = np.nan
    own = rng.random(shape) < rng.uniform(0.0, 0.1, (shape[0], 1))  # 0 to about 6 owning lanes per wave
    with np.errstate(invalid="ignore"):
        take = _shipped(u, v) & own
        cand1 = _first_exit_keeps(u) & own
        cand2 = cand1 & _second_exit_keeps(u, v)
    exit1, exit2 = ~cand1.any(axis=1), ~cand2.any(axis=1)
    assert 1000 < exit1.sum() < shape[0] - 1000 and exit2.sum() > exit1.sum()  # both outcomes are exercised
    assert not take[exit1].any()
    assert not take[exit2].any()
