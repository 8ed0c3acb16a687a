"""The neighbourhood guard of rt_render_adaptive_guarded, the CPU side: the rule in numpy, its
prediction on the oracle's samples, and the ABI.

The own-pixel test is tests/test_adaptive_spec.py's `converged`, unchanged.  After each pass
  fail[q] = active[q] and not own_test(q)
and an active pixel p retires iff no q with |qx - px| <= r and |qy - py| <= r inside the
rendered rectangle has fail[q] (the window is clipped to the rectangle; nothing outside it
exists).  A retired pixel never fails — its moments are frozen and it passed on them — and
never returns; at the cap every active pixel stops.  tests/test_gpu_adaptive_guard.py imports
`guard_retire` and `predict_guarded` and compares the GPU's maps with them for equality.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle as O
import rtnw
from conftest import ROOT
from test_adaptive_spec import converged, moments_f32, spp_schedule

RT_ERR_INVALID = -1
SEED = 19
THREADS = min(16, os.cpu_count() or 1)


# ------------------------------------------------------------------ the rule, in numpy
def guard_retire(active, own, radius):
    """Steps 2-3: the pixels [h, w] that leave the active set after a pass.  active: the set
    before; own: the own-pixel test of every pixel (read only where active)."""
    active = np.asarray(active, bool)
    fail = active & ~np.asarray(own, bool)
    h, w = fail.shape
    r = int(radius)
    held = np.zeros((h, w), bool)
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)   # outside the rectangle: nothing fails
    pad[r:r + h, r:r + w] = fail
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            held |= pad[dy:dy + h, dx:dx + w]
    return active & ~held


def ysum(v):
    """y = (r + g) + b in float32."""
    v = np.asarray(v, np.float32)
    return ((v[..., 0] + v[..., 1]).astype(np.float32) + v[..., 2]).astype(np.float32)


def predict_guarded(one, mn, step, cap, tol, floor, r):
    """The guarded rule on one-sample images one[k] ([h, w, 3], sample k of every pixel):
    (spp map, moments at each pixel's own count, held), held = the pixels that at some pass
    before the cap were active, passed their own test and were kept by a neighbour."""
    y = ysum(one)
    spp = np.full(y.shape[1:], cap, np.int32)
    mom = np.zeros(y.shape[1:] + (2,), np.float32)
    active = np.ones(y.shape[1:], bool)
    held = np.zeros(y.shape[1:], bool)
    for n in spp_schedule(mn, step, cap):
        m1, m2 = moments_f32(y[:n])
        own = converged(n, m1, m2, tol, floor)
        retire = guard_retire(active, own, r)
        if n < cap:
            held |= active & own & ~retire
        stop = active & (retire | (n == cap))
        spp[stop] = n
        mom[stop] = np.stack([m1, m2], axis=-1)[stop]
        active &= ~stop
    assert not active.any()
    return spp, mom, held


def test_radius_zero_retires_the_pixels_that_pass():
    rng = np.random.default_rng(1)
    for _ in range(8):
        active, own = rng.random((7, 9)) < 0.7, rng.random((7, 9)) < 0.5
        assert np.array_equal(guard_retire(active, own, 0), active & own)


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("fy,fx", [(3, 4), (0, 4), (3, 8), (0, 0), (6, 8)])   # centre, edges, corners
def test_one_failing_pixel_holds_its_clipped_window(fy, fx, r):
    h, w = 7, 9
    active = np.ones((h, w), bool)
    own = np.ones((h, w), bool)
    own[fy, fx] = False
    want = np.zeros((h, w), bool)
    want[max(0, fy - r):min(h, fy + r + 1), max(0, fx - r):min(w, fx + r + 1)] = True
    kept = ~guard_retire(active, own, r)
    assert np.array_equal(kept, want)
    n_want = (min(h, fy + r + 1) - max(0, fy - r)) * (min(w, fx + r + 1) - max(0, fx - r))
    assert int(kept.sum()) == n_want <= (2 * r + 1) ** 2
    if (fy, fx) == (3, 4):
        assert n_want == (2 * r + 1) ** 2


def test_radius_8_on_a_3_by_2_frame_holds_everything():
    active = np.ones((2, 3), bool)
    for fy in range(2):
        for fx in range(3):
            own = np.ones((2, 3), bool)
            own[fy, fx] = False
            assert not guard_retire(active, own, 8).any()
    assert guard_retire(active, np.ones((2, 3), bool), 8).all()


def test_a_retired_pixel_never_fails():
    # own = False on a pixel that is not active holds nobody: fail is masked by active
    active = np.ones((5, 5), bool)
    active[2, 2] = False
    own = np.ones((5, 5), bool)
    own[2, 2] = False
    for r in (0, 1, 2, 8):
        assert np.array_equal(guard_retire(active, own, r), active)


# ------------------------------------------------------------------ on the oracle's samples
_one = {}


def oracle_samples(scene, nx, ny, n):
    """[n, ny, nx, 3]: the oracle's one-sample images, sample k at sample_offset = k."""
    key = (scene, nx, ny)
    if key not in _one or _one[key].shape[0] < n:
        one = np.stack([O.render(O.kernel_spec(scene, nx, ny, 1, seed=SEED, chunk=1, sample_offset=k, threads=THREADS))[0]
                        for k in range(n)])
        one.setflags(write=False)
        _one[key] = one
    return _one[key][:n]


def count_map(spp):
    return {int(n): int((spp == n).sum()) for n in np.unique(spp)}


# (scene, nx, ny, tol, r, populated counts asked for): all with (min, step, cap) = (4, 4, 16), floor 0.01
CASES = [("random_motion", 16, 16, 0.5, 1, 3), ("random_motion", 24, 16, 0.5, 2, 3), ("final", 16, 16, 0.25, 1, 2)]


@pytest.mark.parametrize("scene,nx,ny,tol,r,populated", CASES)
def test_the_guarded_maps_of_the_oracles_samples_are_not_trivial(scene, nx, ny, tol, r, populated):
    one = oracle_samples(scene, nx, ny, 16)
    spp, mom, held = predict_guarded(one, 4, 4, 16, tol, 0.01, r)
    spp0, mom0, held0 = predict_guarded(one, 4, 4, 16, tol, 0.01, 0)
    counts = count_map(spp)
    print(f"{scene} {nx}x{ny} tol {tol} r {r}: {counts}, held {int(held.sum())}; r = 0: {count_map(spp0)}")
    assert sum(1 for c in counts.values() if c >= 16) >= populated, counts
    assert int(held.sum()) >= 64
    # radius 0 holds nobody, and the guard only ever adds samples
    assert not held0.any()
    assert (spp >= spp0).all() and (spp > spp0).any()
    # a pixel's moments are those of its own count
    for n in counts:
        m1, m2 = moments_f32(ysum(one[:n]))
        sel = spp == n
        assert np.array_equal(mom[sel].view(np.uint32), np.stack([m1, m2], -1)[sel].view(np.uint32))


def test_radius_zero_on_the_oracles_samples_is_the_unguarded_rule():
    # each pixel stops at the first count of the schedule at which its own test passes
    # (tests/test_gpu_adaptive.py quotes {4: 104, 8: 40, 12: 47, 16: 65} for these inputs)
    one = oracle_samples("random_motion", 16, 16, 16)
    spp, _, held = predict_guarded(one, 4, 4, 16, 0.25, 0.01, 0)
    want = np.full(spp.shape, 16, np.int32)
    for n in reversed(spp_schedule(4, 4, 16)[:-1]):
        want[converged(n, *moments_f32(ysum(one[:n])), 0.25, 0.01)] = n
    print(count_map(spp))
    assert np.array_equal(spp, want) and not held.any()
    assert len(count_map(spp)) >= 3


# ------------------------------------------------------------------ the ABI
def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_header_and_library_have_the_guarded_entry_point():
    L = rtnw.lib()
    assert "rt_render_adaptive_guarded" in set(rtnw.header_symbols())
    for name in ("rt_render_adaptive_guarded", "rt_render_adaptive", "rt_launch_adaptive_test", "rt_launch_adaptive_guard",
                 "rt_launch_adaptive_select"):
        assert hasattr(L, name), name
    assert L.rt_render_adaptive_guarded.argtypes is not None
    assert re.search(r"#define RT_ABI_VERSION 2\b", _header())
    assert ctypes.sizeof(rtnw.RtAdaptiveParams) == 16


def _guarded(params, ap, radius):
    """rt_render_adaptive_guarded with a null scene (test_adaptive_spec._adaptive's pattern):
    every argument check comes before any HIP call, the scene's last."""
    L = rtnw.lib()
    camd = rtnw.RtCameraDesc()
    buf = np.zeros((2, 2, 3), np.float32)
    rc = L.rt_render_adaptive_guarded(None, ctypes.byref(camd), ctypes.byref(params), ctypes.byref(ap), radius, 0, 0, 2, 2,
                                      buf.ctypes.data, None, None, None)
    return rc, L.rt_last_error().decode()


def _good():
    return (rtnw.RenderParams(2, 2, 16, seed=1),
            rtnw.RtAdaptiveParams(min_spp=4, step_spp=4, tolerance=0.25, floor=0.01))


@pytest.mark.parametrize("radius", [-1, 9])
def test_a_radius_outside_0_to_8_is_invalid(radius):
    rc, msg = _guarded(*_good(), radius)
    assert rc == RT_ERR_INVALID and "radius" in msg and "null scene" not in msg, msg


@pytest.mark.parametrize("radius", [0, 1, 8])
def test_valid_arguments_reach_the_scene_check(radius):
    rc, msg = _guarded(*_good(), radius)
    assert rc == RT_ERR_INVALID and "null scene" in msg and "rt_render_adaptive_guarded" in msg, msg


def test_the_other_checks_are_rt_render_adaptives():
    p, a = _good()
    a.min_spp = 1
    rc, msg = _guarded(p, a, 1)
    assert rc == RT_ERR_INVALID and "min_spp" in msg, msg
    p, a = _good()
    p.flags = rtnw.RT_FLAG_SUM_IN
    rc, msg = _guarded(p, a, 1)
    assert rc == RT_ERR_INVALID and "RT_FLAG_SUM_IN" in msg, msg
