"""Adaptive sampling on the GPU: rt_render_tiles_moments and rt_render_adaptive.

Everything is checked for EQUALITY.  The counter RNG is keyed by (pixel, sample), so a
one-sample render at sample_offset = k (the existing rt_render_tile) is sample k's radiance;
from those images numpy restates, in float32 and in sample order, the sums and the moments
the new resolve keeps, and — with the rule of tests/test_adaptive_spec.py — the sample count
at which every pixel stops.  A pixel that stopped at n must be that pixel of the fixed
n-spp render, bit for bit.
"""
import numpy as np
import pytest

import oracle as O
import rtnw
from test_adaptive_spec import converged, moments_f32, spp_schedule
from test_gpu_parity import THREADS, TOL_RMS, _scene, assert_exact, gamma_rms

pytestmark = pytest.mark.gpu

SEED = 19
FOLD, SUM_IN, SUM_OUT = rtnw.RT_FLAG_RIGHT_FOLD, rtnw.RT_FLAG_SUM_IN, rtnw.RT_FLAG_SUM_OUT


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def setup(scene, nx, ny, ns, **kw):
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    kw.setdefault("chunk", 1)
    p = rtnw.RenderParams(nx, ny, ns, max_depth=depth, background=bg, seed=SEED, **kw)
    return _scene(scene), rtnw.Camera.preset(cam_name, nx, ny), p


def fixed(scene, nx, ny, ns, rect=None, **kw):
    sc, cam, p = setup(scene, nx, ny, ns, **kw)
    return sc.render_tile(cam, p, *(rect or (0, 0, nx, ny)))


_samples = {}


def samples(scene, nx, ny, n, rect=None):
    """[n, h, w, 3]: sample k's radiance of every pixel, from n one-sample renders
    (spp = 1, sample_offset = k) of the existing rt_render_tile.  Computed once, never written."""
    key = (scene, nx, ny, rect)
    have = _samples.get(key)
    if have is None or have.shape[0] < n:
        have = np.stack([fixed(scene, nx, ny, 1, rect, sample_offset=k) for k in range(n)])
        have.setflags(write=False)
        _samples[key] = have
    return have[:n]


def ysum(v):
    """y = (r + g) + b in float32."""
    v = np.asarray(v, np.float32)
    return ((v[..., 0] + v[..., 1]).astype(np.float32) + v[..., 2]).astype(np.float32)


def np_moments(items):
    """[h, w, 2] float32 moments of the items' y, in item order."""
    m1, m2 = moments_f32(ysum(items))
    return np.stack([m1, m2], axis=-1)


def np_sums(items):
    s = np.zeros(items.shape[1:], np.float32)
    for v in items:
        s = (s + v).astype(np.float32)
    return s


# ---- 1. moments, bitwise --------------------------------------------------------------
@pytest.mark.parametrize("scene", ["final", "random_motion", "cornell_smoke", "cornell_box"])
def test_moments_are_the_float32_sums_of_the_samples(scene):
    nx = ny = 16
    ns = 8
    sc, cam, p = setup(scene, nx, ny, ns)
    out, mom, st = sc.render_tile_moments(cam, p, 0, 0, nx, ny, stats=True)
    assert st["chunk"] == 1 and st["samples"] == nx * ny * ns
    assert same(out, fixed(scene, nx, ny, ns))                   # bitwise what rt_render_tile writes
    one = samples(scene, nx, ny, ns)
    assert same((np_sums(one) * np.float32(1.0 / ns)).astype(np.float32), out)
    assert same(np_moments(one), mom)
    assert (mom[..., 1] > 0).any()                               # not a black frame
    # the oracle's own one-sample images: summed in order they are its 8-spp image (CPU, always
    # exact), and their moments are the GPU's under the parity suite's convention
    o_one = np.stack([O.render(O.kernel_spec(scene, nx, ny, 1, seed=SEED, chunk=1, sample_offset=k, threads=THREADS))[0]
                      for k in range(ns)])
    o_all = O.render(O.kernel_spec(scene, nx, ny, ns, seed=SEED, chunk=1, threads=THREADS))[0]
    assert same((np_sums(o_one) * np.float32(1.0 / ns)).astype(np.float32), o_all)
    assert (gamma_rms(out, o_all) <= TOL_RMS).all()
    exact = float(np.mean(np.all(bits(np_moments(o_one)) == bits(mom), axis=-1)))
    print(f"{scene}: moments bit-exact against the oracle on {exact:.4f} of the pixels")
    assert_exact(exact)


def test_moments_with_two_items_per_pixel():
    """chunk 4 at 8 spp: y is the channel sum of each ITEM's partial sum, two items per pixel."""
    scene, nx, ny = "final", 16, 16
    sc, cam, p = setup(scene, nx, ny, 8, chunk=4)
    out, mom = sc.render_tile_moments(cam, p, 0, 0, nx, ny)
    assert same(out, fixed(scene, nx, ny, 8, chunk=4))
    items = np.stack([fixed(scene, nx, ny, 4, chunk=4, sample_offset=k, flags=SUM_OUT) for k in (0, 4)])
    assert same(np_moments(items), mom)
    assert not same(np_moments(samples(scene, nx, ny, 8)), mom)   # not the per-sample moments


def test_moments_of_a_tile_inside_a_larger_frame():
    scene, nx, ny, rect = "final", 24, 16, (3, 5, 13, 7)
    sc, cam, p = setup(scene, nx, ny, 8)
    out, mom = sc.render_tile_moments(cam, p, *rect)
    assert out.shape == (7, 13, 3) and mom.shape == (7, 13, 2)
    assert same(out, fixed(scene, nx, ny, 8, rect))
    assert same(np_moments(samples(scene, nx, ny, 8, rect)), mom)


def test_moments_do_not_depend_on_the_sample_batches(monkeypatch):
    scene, nx, ny, ns = "final", 16, 16, 16
    sc, cam, p = setup(scene, nx, ny, ns)
    out, mom, st = sc.render_tile_moments(cam, p, 0, 0, nx, ny, stats=True)
    assert st["batches"] == 1
    monkeypatch.setenv("RTNW_SLAB_BUDGET", str(nx * ny * 12 * 6))   # room for 6 of the 16 samples
    out_b, mom_b, st_b = sc.render_tile_moments(cam, p, 0, 0, nx, ny, stats=True)
    assert st_b["batches"] >= 3
    assert same(out_b, out) and same(mom_b, mom)
    assert same(np_moments(samples(scene, nx, ny, ns)), mom)


def test_moments_continue_with_sum_in():
    scene, nx, ny = "random_motion", 16, 16
    sc, cam, p16 = setup(scene, nx, ny, 16)
    out16, mom16 = sc.render_tile_moments(cam, p16, 0, 0, nx, ny)
    _, _, pa = setup(scene, nx, ny, 8, flags=SUM_OUT)
    sums8, mom8 = sc.render_tile_moments(cam, pa, 0, 0, nx, ny)
    assert same(sums8, np_sums(samples(scene, nx, ny, 8))) and same(mom8, np_moments(samples(scene, nx, ny, 8)))
    _, _, pb = setup(scene, nx, ny, 8, flags=SUM_IN, sample_offset=8)
    out, mom = sc.render_tile_moments(cam, pb, 0, 0, nx, ny, sums=sums8, moments=mom8)
    assert same(out, out16) and same(mom, mom16)
    assert same(out16, fixed(scene, nx, ny, 16))


# ---- 2. no convergence: the fixed render ------------------------------------------------
@pytest.mark.parametrize("scene", ["final", "random_motion"])
@pytest.mark.parametrize("mn,step,cap,passes", [(4, 4, 16, 4), (2, 3, 9, 4), (16, 1, 16, 1)])
def test_tolerance_zero_is_the_fixed_render(scene, mn, step, cap, passes):
    nx = ny = 16
    sc, cam, p = setup(scene, nx, ny, cap, chunk=0)
    img, spp, mom, st = sc.render_adaptive(cam, p, 0, 0, nx, ny, min_spp=mn, step_spp=step, tolerance=0.0, floor=0.01)
    assert same(img, fixed(scene, nx, ny, cap))
    assert (spp == cap).all()
    assert st["samples"] == nx * ny * cap and st["passes"] == passes
    assert st["pixels_converged"] == 0 and st["pixels_capped"] == nx * ny
    assert same(mom, np_moments(samples(scene, nx, ny, cap)))


# ---- 3. convergence -------------------------------------------------------------------
def predict(one, mn, step, cap, tol, floor):
    """The rule applied to the GPU's own samples: (spp map, moments at each pixel's own count)."""
    y = ysum(one)
    spp = np.full(y.shape[1:], cap, np.int32)
    mom = np.zeros(y.shape[1:] + (2,), np.float32)
    active = np.ones(y.shape[1:], bool)
    for n in spp_schedule(mn, step, cap):
        m1, m2 = moments_f32(y[:n])
        stop = active & (converged(n, m1, m2, tol, floor) | (n == cap))
        spp[stop] = n
        mom[stop] = np.stack([m1, m2], axis=-1)[stop]
        active &= ~stop
    assert not active.any()
    return spp, mom


def check_adaptive(scene, nx, ny, mn, step, cap, tol, floor, rect=None):
    sc, cam, p = setup(scene, nx, ny, cap)
    x0, y0, w, h = rect or (0, 0, nx, ny)
    img, spp, mom, st = sc.render_adaptive(cam, p, x0, y0, w, h, min_spp=mn, step_spp=step, tolerance=tol, floor=floor)
    want_spp, want_mom = predict(samples(scene, nx, ny, cap, rect), mn, step, cap, tol, floor)
    counts = {int(n): int((spp == n).sum()) for n in np.unique(spp)}
    print(f"{scene} ({mn},{step},{cap}) tol {tol} floor {floor}: spp map {counts}, stats {st}")
    assert np.array_equal(spp, want_spp)
    assert same(mom, want_mom)
    for n in counts:                       # every pixel is that pixel of the fixed n-spp render
        sel = spp == n
        assert np.array_equal(bits(img)[sel], bits(fixed(scene, nx, ny, n, rect))[sel]), n
    assert st["samples"] == int(spp.sum())
    assert st["passes"] == spp_schedule(mn, step, cap).index(int(spp.max())) + 1
    assert st["pixels_converged"] + st["pixels_capped"] == w * h
    return img, spp, mom, counts


@pytest.mark.parametrize("mn,step,cap,tol,floor", [(4, 4, 16, 0.25, 0.01), (2, 3, 9, 0.3, 0.01)])
def test_converged_pixels_are_the_fixed_render_at_their_own_count(mn, step, cap, tol, floor):
    # the oracle alone gives {4: 104, 8: 40, 12: 47, 16: 65} and {2: 141, 5: 32, 8: 26, 9: 57}
    _, _, _, counts = check_adaptive("random_motion", 16, 16, mn, step, cap, tol, floor)
    assert sum(1 for c in counts.values() if c >= 16) >= 3, counts   # the map is not trivial


def test_convergence_on_final():
    check_adaptive("final", 16, 16, 4, 4, 16, 0.25, 0.01)   # the oracle alone: {4: 229, 8: 4, 16: 23}


# ---- 4. invariances -------------------------------------------------------------------
def test_two_runs_are_identical_and_a_tile_is_the_crop_of_the_frame():
    scene, nx, ny, rect = "random_motion", 24, 16, (3, 5, 13, 7)
    a = check_adaptive(scene, nx, ny, 4, 4, 16, 0.25, 0.01)
    sc, cam, p = setup(scene, nx, ny, 16)
    b = sc.render_adaptive(cam, p, 0, 0, nx, ny, min_spp=4, step_spp=4, tolerance=0.25, floor=0.01)
    assert same(a[0], b[0]) and np.array_equal(a[1], b[1]) and same(a[2], b[2])
    x0, y0, w, h = rect
    t = check_adaptive(scene, nx, ny, 4, 4, 16, 0.25, 0.01, rect)
    assert len(t[3]) >= 2   # pixels that stopped early and late (the oracle alone: {4: 27, 8: 15, 12: 22, 16: 27})
    for whole, part in zip(a[:3], t[:3]):
        assert np.array_equal(bits(whole[y0:y0 + h, x0:x0 + w]), bits(part))


def test_right_fold_passes_through():
    scene, nx, ny = "final", 16, 16
    sc, cam, p = setup(scene, nx, ny, 8, chunk=0, flags=FOLD)
    img, spp, _, st = sc.render_adaptive(cam, p, 0, 0, nx, ny, min_spp=4, step_spp=4, tolerance=0.0, floor=0.0)
    assert (spp == 8).all() and st["passes"] == 2
    assert same(img, fixed(scene, nx, ny, 8, chunk=0, flags=FOLD))
    assert not same(img, fixed(scene, nx, ny, 8))               # the fold image is not the forward one
