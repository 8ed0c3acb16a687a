"""The denoiser on the GPU: rt_denoise and rt_denoise_dev equal the numpy statement of
tests/test_denoise_spec.py bit for bit, on synthetic inputs and on rendered ones, and the
filtered image of a few-sample render is closer to a many-sample reference than the input.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_denoise_spec import denoise_ref, synthetic
from test_gpu_parity import _scene, gamma_rms

pytestmark = pytest.mark.gpu

SIGMAS = dict(sigma_color=4.0, sigma_depth=1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def mismatch(a, b):
    d = bits(a) != bits(b)
    return f"{int(d.sum())} of {d.size} values differ, largest difference {float(np.abs(a - b).max()):.3g}"


_inputs = {}


def inputs(nx, ny):
    if (nx, ny) not in _inputs:
        d = synthetic(nx, ny, 100 * nx + ny)
        for v in d.values():
            v.setflags(write=False)
        _inputs[(nx, ny)] = d
    return _inputs[(nx, ny)]


def moment_args(d, mode):
    """(moments, spp) of the three ways the filter is driven."""
    return {"map": (d["moments"], d["spp"]), "uniform": (d["moments"], 8), "none": (None, None)}[mode]


@pytest.mark.parametrize("mode", ["map", "uniform", "none"])
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
@pytest.mark.parametrize("nx,ny", [(1, 1), (17, 13), (64, 3), (33, 40)])
def test_denoise_equals_the_statement(nx, ny, iterations, demodulate, mode):
    d = inputs(nx, ny)
    mom, spp = moment_args(d, mode)
    kw = dict(iterations=iterations, demodulate=demodulate, **SIGMAS)
    got = rtnw.denoise(d["color"], d, mom, spp, **kw)
    want = denoise_ref(d["color"], d["albedo"], d["normal"], d["depth"], mom, spp, **kw)
    assert np.isfinite(want).all()
    assert same(got, want), mismatch(got, want)


@pytest.mark.parametrize("mode", ["map", "uniform", "none"])
@pytest.mark.parametrize("iterations", [0, 3])
def test_device_entry_point_equals_the_host_one(iterations, mode):
    nx, ny = 33, 40
    d = inputs(nx, ny)
    mom, spp = moment_args(d, mode)
    kw = dict(iterations=iterations, demodulate=1, **SIGMAS)
    want = rtnw.denoise(d["color"], d, mom, spp, **kw)
    guides = np.zeros((ny, nx, 8), np.float32)
    guides[..., 0:3], guides[..., 4:7], guides[..., 7] = d["albedo"], d["normal"], d["depth"]
    L = rtnw.lib()
    parts = [np.ascontiguousarray(d["color"]), guides]
    if mom is not None:
        parts.append(np.ascontiguousarray(mom))
        if np.ndim(spp):
            parts.append(np.ascontiguousarray(spp))
    out = np.zeros((ny, nx, 3), np.float32)
    sizes = [a.nbytes for a in parts] + [out.nbytes]
    dev = ctypes.c_void_p()
    rtnw._check(L.rt_device_alloc(0, sum(sizes), ctypes.byref(dev)))
    try:
        ptr, off = [], 0
        for a in parts:
            rtnw._check(L.rt_copy_to_device(ctypes.c_void_p(dev.value + off), a.ctypes.data, a.nbytes))
            ptr.append(dev.value + off)
            off += a.nbytes
        dp = rtnw.denoise_params(uniform_spp=0 if np.ndim(spp) or spp is None else spp, **kw)
        rtnw._check(L.rt_denoise_dev(0, nx, ny, ptr[0], ptr[1], ptr[2] if mom is not None else None,
                                     ptr[3] if len(ptr) > 3 else None, ctypes.byref(dp), dev.value + off, None))
        rtnw._check(L.rt_copy_to_host(out.ctypes.data, ctypes.c_void_p(dev.value + off), out.nbytes))
    finally:
        L.rt_device_free(dev)
    assert same(out, want), mismatch(out, want)


_reference = {}


def reference(nx, ny):
    """512 spp with another seed: the yardstick of DESIGN.md §7b.  Rendered once."""
    if (nx, ny) not in _reference:
        cam_name, bg, depth = rtnw.SCENE_DEFAULTS["random_scene"]
        p = rtnw.RenderParams(nx, ny, 512, max_depth=depth, background=bg, seed=977, chunk=1)
        img = _scene("random_scene").render_tile(rtnw.Camera.preset(cam_name, nx, ny), p, 0, 0, nx, ny)
        img.setflags(write=False)
        _reference[(nx, ny)] = img
    return _reference[(nx, ny)]


@pytest.mark.parametrize("adaptive", [False, True])
def test_pipeline_on_rendered_data(adaptive):
    nx, ny, n = 48, 32, 8
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS["random_scene"]
    sc, cam = _scene("random_scene"), rtnw.Camera.preset(cam_name, nx, ny)
    p = rtnw.RenderParams(nx, ny, n, max_depth=depth, background=bg, seed=31, chunk=1)
    if adaptive:
        color, spp, mom, _ = sc.render_adaptive(cam, p, 0, 0, nx, ny, min_spp=4, step_spp=2, tolerance=0.1, floor=0.01)
        assert spp.min() >= 4 and spp.max() <= n
    else:
        color, mom = sc.render_tile_moments(cam, p, 0, 0, nx, ny)
        spp = n
    f = sc.render_features(cam, p, 0, 0, nx, ny)
    kw = dict(rtnw.DENOISE_DEFAULTS)
    got = rtnw.denoise(color, f, mom, spp, **kw)
    want = denoise_ref(color, f["albedo"], f["normal"], f["depth"], mom, spp, **kw)
    assert same(got, want), mismatch(got, want)
    ref = reference(nx, ny)
    before, after = float(gamma_rms(color, ref).mean()), float(gamma_rms(got, ref).mean())
    print(f"random_scene {nx}x{ny}, {'adaptive 4..8' if adaptive else 'fixed 8'} spp: gamma RMS against 512 spp "
          f"{before:.4f} -> {after:.4f} denoised")
    assert after < before
