"""The denoiser's variance pre-filter on the GPU: rt_denoise and rt_denoise_dev with
rt_denoise_params.variance_filter = 1 equal tests/test_denoise_varfilter_spec.py's numpy
statement bit for bit, on synthetic inputs and on rendered ones; with 0 they equal the
filter of tests/test_denoise_spec.py.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_denoise_spec import denoise_ref
from test_denoise_varfilter_spec import denoise_vf_ref
from test_gpu_denoise import SIGMAS, inputs, mismatch, moment_args, reference, same
from test_gpu_parity import _scene, gamma_rms

pytestmark = pytest.mark.gpu


def statement(d, mom, spp, **kw):
    return denoise_vf_ref(d["color"], d["albedo"], d["normal"], d["depth"], mom, spp, **kw)


@pytest.mark.parametrize("mode", ["map", "uniform", "none"])
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("nx,ny", [(1, 1), (5, 3), (64, 4), (65, 5), (33, 40)])
def test_variance_filter_equals_the_statement(nx, ny, iterations, mode):
    d = inputs(nx, ny)
    mom, spp = moment_args(d, mode)
    kw = dict(iterations=iterations, demodulate=1, **SIGMAS)
    got = rtnw.denoise(d["color"], d, mom, spp, variance_filter=1, **kw)
    want = statement(d, mom, spp, variance_filter=1, **kw)
    assert np.isfinite(want).all()
    assert same(got, want), mismatch(got, want)
    off = rtnw.denoise(d["color"], d, mom, spp, variance_filter=0, **kw)
    if mode == "none":
        assert same(got, off)                       # without moments the switch has no effect
    elif nx * ny > 1:
        assert not same(got, off)                   # with them it is a different filter


@pytest.mark.parametrize("mode", ["map", "uniform", "none"])
@pytest.mark.parametrize("nx,ny", [(17, 13), (33, 40)])
def test_variance_filter_0_is_the_filter_of_before(nx, ny, mode):
    d = inputs(nx, ny)
    mom, spp = moment_args(d, mode)
    kw = dict(iterations=3, demodulate=1, **SIGMAS)
    got = rtnw.denoise(d["color"], d, mom, spp, variance_filter=0, **kw)
    want = denoise_ref(d["color"], d["albedo"], d["normal"], d["depth"], mom, spp, **kw)
    assert same(got, want), mismatch(got, want)
    assert same(got, rtnw.denoise(d["color"], d, mom, spp, **kw))


@pytest.mark.parametrize("mode", ["map", "uniform", "none"])
def test_device_entry_point_equals_the_host_one(mode):
    nx, ny = 33, 40
    d = inputs(nx, ny)
    mom, spp = moment_args(d, mode)
    kw = dict(iterations=3, demodulate=1, **SIGMAS)
    want = rtnw.denoise(d["color"], d, mom, spp, variance_filter=1, **kw)
    guides = np.zeros((ny, nx, 8), np.float32)
    guides[..., 0:3], guides[..., 4:7], guides[..., 7] = d["albedo"], d["normal"], d["depth"]
    L = rtnw.lib()
    parts = [np.ascontiguousarray(d["color"]), guides]
    if mom is not None:
        parts.append(np.ascontiguousarray(mom))
        if np.ndim(spp):
            parts.append(np.ascontiguousarray(spp))
    out = np.zeros((ny, nx, 3), np.float32)
    dev = ctypes.c_void_p()
    rtnw._check(L.rt_device_alloc(0, sum(a.nbytes for a in parts) + out.nbytes, ctypes.byref(dev)))
    try:
        ptr, off = [], 0
        for a in parts:
            rtnw._check(L.rt_copy_to_device(ctypes.c_void_p(dev.value + off), a.ctypes.data, a.nbytes))
            ptr.append(dev.value + off)
            off += a.nbytes
        dp = rtnw.denoise_params(uniform_spp=0 if np.ndim(spp) or spp is None else spp, variance_filter=1, **kw)
        rtnw._check(L.rt_denoise_dev(0, nx, ny, ptr[0], ptr[1], ptr[2] if mom is not None else None,
                                     ptr[3] if len(ptr) > 3 else None, ctypes.byref(dp), dev.value + off, None))
        rtnw._check(L.rt_copy_to_host(out.ctypes.data, ctypes.c_void_p(dev.value + off), out.nbytes))
    finally:
        L.rt_device_free(dev)
    assert same(out, want), mismatch(out, want)


@pytest.mark.parametrize("adaptive", [False, True])
def test_pipeline_on_rendered_data(adaptive):
    nx, ny, n = 48, 32, 8
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS["random_scene"]
    sc, cam = _scene("random_scene"), rtnw.Camera.preset(cam_name, nx, ny)
    p = rtnw.RenderParams(nx, ny, n, max_depth=depth, background=bg, seed=31, chunk=1)
    if adaptive:
        color, spp, mom, _ = sc.render_adaptive(cam, p, 0, 0, nx, ny, min_spp=4, step_spp=2, tolerance=0.1, floor=0.01,
                                                guard_radius=1)
        assert spp.min() >= 4 and spp.max() <= n
    else:
        color, mom = sc.render_tile_moments(cam, p, 0, 0, nx, ny)
        spp = n
    f = sc.render_features(cam, p, 0, 0, nx, ny)
    kw = dict(rtnw.DENOISE_DEFAULTS)
    ref = reference(nx, ny)
    rms = {"input": float(gamma_rms(color, ref).mean())}
    for vf in (0, 1):
        got = rtnw.denoise(color, f, mom, spp, variance_filter=vf, **kw)
        want = denoise_vf_ref(color, f["albedo"], f["normal"], f["depth"], mom, spp, variance_filter=vf, **kw)
        assert same(got, want), (vf, mismatch(got, want))
        rms[vf] = float(gamma_rms(got, ref).mean())
    print(f"random_scene {nx}x{ny}, {'adaptive 4..8 guarded r 1' if adaptive else 'fixed 8'} spp: gamma RMS against "
          f"512 spp {rms['input']:.4f} -> {rms[0]:.4f} denoised -> {rms[1]:.4f} with the variance pre-filter")
