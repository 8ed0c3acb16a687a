"""rt_render_adaptive_guarded on the GPU: the guard kernel against the numpy statement on
random masks, and the guarded render against `predict_guarded` applied to the GPU's own
one-sample renders (tests/test_adaptive_guard_spec.py) — everything for EQUALITY, as in
tests/test_gpu_adaptive.py, whose harness this file reuses.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_adaptive_guard_spec import CASES, count_map, guard_retire, predict_guarded
from test_adaptive_spec import spp_schedule
from test_gpu_adaptive import FOLD, bits, fixed, np_moments, same, samples, setup
from test_gpu_parity import gamma_rms

pytestmark = pytest.mark.gpu


# ---- 1. the guard kernel alone -----------------------------------------------------------
def _guard_launcher():
    fn = rtnw.lib().rt_launch_adaptive_guard
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p]
    return fn


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (63, 3), (64, 4), (65, 5), (130, 9), (200, 37)])
def test_guard_kernel_equals_the_statement(w, h):
    """A partial wave, a block edge inside a row, a halo that spans three blocks (130 wide),
    frames smaller than the window; densities 0, 0.02, 0.3, 1 of failing pixels; r = 0, 1, 2, 8."""
    L, guard = rtnw.lib(), _guard_launcher()
    npix = w * h
    plane = (npix + 15) // 16 * 16
    dev = ctypes.c_void_p()
    rtnw._check(L.rt_device_alloc(0, 2 * plane + 16, ctypes.byref(dev)))
    d_fail, d_act, d_cnt = dev.value, dev.value + plane, dev.value + 2 * plane
    rng = np.random.default_rng(1000 * w + h)
    try:
        for density in (0.0, 0.02, 0.3, 1.0):
            active = rng.random((h, w)) < 0.8
            if density == 1.0:
                active[:] = True
            fail = active & (rng.random((h, w)) < density if density < 1.0 else True)
            for r in (0, 1, 2, 8):
                want_retire = guard_retire(active, ~fail, r)
                want_active = active & ~want_retire
                f8, a8, cnt = fail.astype(np.uint8), active.astype(np.uint8), np.zeros(4, np.uint32)
                for dst, src in ((d_fail, f8), (d_act, a8), (d_cnt, cnt)):
                    rtnw._check(L.rt_copy_to_device(ctypes.c_void_p(dst), src.ctypes.data, src.nbytes))
                assert guard(w, h, r, d_fail, d_act, d_cnt, None) == 0
                got, gcnt = np.zeros((h, w), np.uint8), np.zeros(4, np.uint32)
                rtnw._check(L.rt_copy_to_host(got.ctypes.data, ctypes.c_void_p(d_act), got.nbytes))
                rtnw._check(L.rt_copy_to_host(gcnt.ctypes.data, ctypes.c_void_p(d_cnt), gcnt.nbytes))
                where = f"{w}x{h} density {density} r {r}"
                assert np.array_equal(got, want_active.astype(np.uint8)), where
                assert (int(gcnt[0]), int(gcnt[1])) == (int(want_active.sum()), int(want_retire.sum())), where
                if density == 0.0:
                    assert not got.any(), where                         # nobody fails: everyone retires
                if density == 1.0 or (r == 8 and w <= 9 and h <= 9 and fail.any()):
                    assert np.array_equal(got, a8), where               # a failing pixel in every window
    finally:
        L.rt_device_free(dev)


def test_guard_launcher_refuses_a_radius_it_has_no_room_for():
    guard = _guard_launcher()
    assert guard(4, 4, 9, None, None, None, None) != 0 and guard(4, 4, -1, None, None, None, None) != 0


# ---- 2. the guarded render -----------------------------------------------------------------
def render(scene, nx, ny, mn, step, cap, tol, floor, r, rect=None, **kw):
    sc, cam, p = setup(scene, nx, ny, cap, **kw)
    return sc.render_adaptive(cam, p, *(rect or (0, 0, nx, ny)), min_spp=mn, step_spp=step, tolerance=tol, floor=floor,
                              guard_radius=r)


def check_guarded(scene, nx, ny, mn, step, cap, tol, floor, r, rect=None):
    x0, y0, w, h = rect or (0, 0, nx, ny)
    img, spp, mom, st = render(scene, nx, ny, mn, step, cap, tol, floor, r, rect)
    want_spp, want_mom, held = predict_guarded(samples(scene, nx, ny, cap, rect), mn, step, cap, tol, floor, r)
    counts = count_map(spp)
    print(f"{scene} {w}x{h} ({mn},{step},{cap}) tol {tol} floor {floor} r {r}: spp map {counts}, "
          f"held {int(held.sum())}, stats {st}")
    assert np.array_equal(spp, want_spp)
    assert same(mom, want_mom)
    for n in counts:                       # every pixel is that pixel of the fixed n-spp render
        sel = spp == n
        assert np.array_equal(bits(img)[sel], bits(fixed(scene, nx, ny, n, rect))[sel]), n
    assert st["samples"] == int(spp.sum())
    assert st["passes"] == spp_schedule(mn, step, cap).index(int(spp.max())) + 1
    assert st["pixels_converged"] + st["pixels_capped"] == w * h
    # against rt_render_adaptive with the same parameters: never fewer samples, and not the same map
    _, spp0, _, _ = render(scene, nx, ny, mn, step, cap, tol, floor, None, rect)
    assert (spp >= spp0).all()
    assert not np.array_equal(spp, spp0)
    return img, spp, mom, st


@pytest.mark.parametrize("scene,nx,ny,tol,r,populated", CASES)
def test_guarded_render_is_the_statement_on_the_gpus_own_samples(scene, nx, ny, tol, r, populated):
    _, spp, _, _ = check_guarded(scene, nx, ny, 4, 4, 16, tol, 0.01, r)
    assert sum(1 for c in count_map(spp).values() if c >= 16) >= populated


def test_guarded_tile_sees_only_its_own_rectangle():
    scene, nx, ny, rect = "random_motion", 24, 16, (3, 5, 13, 7)
    x0, y0, w, h = rect
    _, t_spp, _, _ = check_guarded(scene, nx, ny, 4, 4, 16, 0.5, 0.01, 2, rect)
    _, f_spp, _, _ = render(scene, nx, ny, 4, 4, 16, 0.5, 0.01, 2)
    # the window is clipped to the rectangle rendered: a tile's pixels never get more than the frame's
    assert (t_spp <= f_spp[y0:y0 + h, x0:x0 + w]).all()


@pytest.mark.parametrize("scene,tol", [("random_motion", 0.25), ("final", 0.25)])
def test_radius_zero_is_rt_render_adaptive(scene, tol):
    a = render(scene, 16, 16, 4, 4, 16, tol, 0.01, None)
    b = render(scene, 16, 16, 4, 4, 16, tol, 0.01, 0)
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1]) and same(a[2], b[2])
    for k in ("passes", "samples", "pixels_converged", "pixels_capped"):
        assert a[3][k] == b[3][k], k
    assert len(count_map(a[1])) >= 2


def test_tolerance_zero_is_the_fixed_render_at_the_cap():
    scene, nx, ny, cap = "random_motion", 16, 16, 16
    img, spp, mom, st = render(scene, nx, ny, 4, 4, cap, 0.0, 0.01, 2, chunk=0)
    assert same(img, fixed(scene, nx, ny, cap)) and (spp == cap).all()
    assert st["samples"] == nx * ny * cap and st["passes"] == 4
    assert st["pixels_converged"] == 0 and st["pixels_capped"] == nx * ny
    assert same(mom, np_moments(samples(scene, nx, ny, cap)))


def test_two_runs_are_identical():
    a = render("random_motion", 24, 16, 4, 4, 16, 0.5, 0.01, 2)
    b = render("random_motion", 24, 16, 4, 4, 16, 0.5, 0.01, 2)
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1]) and same(a[2], b[2]) and a[3]["samples"] == b[3]["samples"]


def test_right_fold_passes_through():
    scene, nx, ny = "final", 16, 16
    img, spp, _, st = render(scene, nx, ny, 4, 4, 8, 0.0, 0.0, 1, chunk=0, flags=FOLD)
    assert (spp == 8).all() and st["passes"] == 2
    assert same(img, fixed(scene, nx, ny, 8, chunk=0, flags=FOLD))
    assert not same(img, fixed(scene, nx, ny, 8))               # the fold image is not the forward one


def test_guard_on_rendered_data_report():
    """Printed, not asserted: what the guard buys on final 32 x 32 against a 512-spp render
    of another seed (DESIGN.md §7d has the full-size tables)."""
    scene, nx, ny = "final", 32, 32
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    sc, cam, _ = setup(scene, nx, ny, 64)
    ref = sc.render_tile(cam, rtnw.RenderParams(nx, ny, 512, max_depth=depth, background=bg, seed=977, chunk=1), 0, 0, nx, ny)
    fx = fixed(scene, nx, ny, 64)
    print(f"{scene} {nx}x{ny}: fixed 64 spp, {nx * ny * 64} samples, gamma RMS against 512 spp "
          f"{float(gamma_rms(fx, ref).mean()):.4f}")
    spent = {}
    for r in (0, 2):
        img, spp, _, st = render(scene, nx, ny, 8, 8, 64, 0.1, 0.01, r)
        spent[r] = int(st["samples"])
        print(f"{scene} {nx}x{ny} adaptive (8,8,64) tol 0.1 r {r}: {spent[r]} samples, {int(st['passes'])} passes, "
              f"gamma RMS against 512 spp {float(gamma_rms(img, ref).mean()):.4f}")
    assert spent[2] >= spent[0]
