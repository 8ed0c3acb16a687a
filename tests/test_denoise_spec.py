"""The denoiser, the CPU side: the ABI's new struct and entry points, the argument checks of
rt_denoise / rt_denoise_dev (made before any HIP call, so they answer without a GPU), and the
exact statement of the filter.

The filter is stated here in numpy float32, not in the product:
tests/test_gpu_denoise.py imports `denoise_ref` and compares the GPU's result with it bit for
bit.  Every operation is an add, subtract, multiply, IEEE divide, max, min or abs on float32
values, in the order written; rt_denoise.hip performs the same sequence without contraction.

One expression differs from the textbook form sum(w e(q)) / sum(w): the filtered colour is
e(p) + sum over q != p of w (e(q) - e(p)) / sum(w), the same value in exact arithmetic, so that
a pixel whose guides reject every neighbour keeps its colour bit for bit (w * e / w does not
return e in float32 for one value in ten).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rtnw
from conftest import ROOT

RT_ERR_INVALID = -1
RT_ERR_HIP = -2
F = np.float32
H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)   # the B3 spline, exact in float32
ALBEDO_MIN = F(0.01)


# ------------------------------------------------------------------ the filter, in numpy
def prepare_ref(color, albedo, moments, spp, demodulate):
    """a', e = c / a' and v, the variance of the mean of the demodulated luminance.
    spp: None (no moments), an int (every pixel's count) or an int32 map."""
    color = np.asarray(color, F)
    a = np.maximum(np.asarray(albedo, F), ALBEDO_MIN) if demodulate else np.ones(color.shape, F)
    e = color / a
    v = np.zeros(color.shape[:2], F)
    if moments is not None:
        m1, m2 = np.asarray(moments, F)[..., 0], np.asarray(moments, F)[..., 1]
        Nf = (np.full(v.shape, spp, np.int32) if np.ndim(spp) == 0 else np.asarray(spp, np.int32)).astype(F)
        s = ((a[..., 0] + a[..., 1]) + a[..., 2]) * F(1.0 / 3.0)
        with np.errstate(all="ignore"):
            var = np.maximum(F(0), m2 - (m1 * m1) / Nf) / ((Nf - F(1)) * Nf) / (s * s)
        v = np.where(Nf >= F(2), var, F(0)).astype(F)   # one sample carries no variance
    return a, e, v


def atrous_ref(n, z, e, v, step, sigma_color, sigma_depth, use_var):
    """One iteration with taps `step` apart: (e', v')."""
    ny, nx = z.shape
    Y, X = np.mgrid[0:ny, 0:nx]
    sc2 = F(sigma_color) * F(sigma_color)
    sz = F(sigma_depth) * F(step)
    lp = (e[..., 0] + e[..., 1]) + e[..., 2]
    lden = sc2 * v + F(1e-8)
    sw = np.zeros((ny, nx), F)
    se = np.zeros((ny, nx, 3), F)
    sv = np.zeros((ny, nx), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx == 0:   # the centre: no edge stopping, no difference to add
                w = H[2] * H[2]
                sw = sw + w
                sv = sv + (w * w) * v
                continue
            qx, qy = X + step * dx, Y + step * dy
            inside = (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
            qx, qy = np.where(inside, qx, X), np.where(inside, qy, Y)   # outside: the centre's data, weight 0
            nq, zq, eq, vq = n[qy, qx], z[qy, qx], e[qy, qx], v[qy, qx]
            wn = np.maximum(F(0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
            for _ in range(7):
                wn = wn * wn
            xz = np.abs(z - zq) / (sz * np.minimum(z, zq) + F(1e-6))
            wz = F(1) / (F(1) + xz * xz)
            w = ((H[dy + 2] * H[dx + 2]) * wn) * wz
            if use_var:
                dl = lp - ((eq[..., 0] + eq[..., 1]) + eq[..., 2])
                w = w * (F(1) / (F(1) + (dl * dl) / lden))
            w = np.where(inside, w, F(0))
            sw = sw + w
            se = se + w[..., None] * (eq - e)
            sv = sv + (w * w) * vq
    assert sw.dtype == se.dtype == sv.dtype == F
    return e + se / sw[..., None], sv / (sw * sw)


def denoise_ref(color, albedo, normal, depth, moments=None, spp=None, *, iterations, demodulate, sigma_color,
                sigma_depth):
    """rt_denoise on host arrays ([ny, nx, ...] float32), bit for bit."""
    color = np.ascontiguousarray(color, F)
    if iterations == 0:
        return color.copy()
    n, z = np.asarray(normal, F), np.asarray(depth, F)
    a, e, v = prepare_ref(color, albedo, moments, spp, demodulate)
    with np.errstate(under="ignore"):
        for i in range(iterations):
            e, v = atrous_ref(n, z, e, v, 1 << i, sigma_color, sigma_depth, moments is not None)
    return e * a


def synthetic(nx, ny, seed):
    """Seeded finite inputs with the blocks the GPU test asks for: zero normals (misses), zero
    variance, and N = 1."""
    rng = np.random.default_rng(seed)
    color = (rng.random((ny, nx, 3)) * 2).astype(F)
    albedo = rng.random((ny, nx, 3)).astype(F)
    albedo[rng.random((ny, nx)) < 0.1] = 0.0               # below the demodulation floor
    # a few plane orientations, slightly perturbed, so that neighbours both agree and disagree
    base = np.array([[0, 1, 0], [1, 0, 0], [0.6, 0.8, 0], [0, 0.6, 0.8]], F)
    normal = (base[rng.integers(0, 4, (ny, nx))] + rng.standard_normal((ny, nx, 3)) * 0.02).astype(F)
    depth = (5 + rng.random((ny, nx)) * 0.5 + 3 * (rng.random((ny, nx)) < 0.2)).astype(F)
    spp = rng.integers(2, 17, (ny, nx)).astype(np.int32)
    ys = (rng.random((16, ny, nx)) * 3).astype(F)
    m1 = np.zeros((ny, nx), F)
    m2 = np.zeros((ny, nx), F)
    for k in range(16):
        use = k < spp
        m1 = np.where(use, m1 + ys[k], m1).astype(F)
        m2 = np.where(use, m2 + ys[k] * ys[k], m2).astype(F)
    by, bx = max(1, ny // 3), max(1, nx // 3)
    normal[:by, :bx] = 0.0                                  # misses: normal 0, depth 0, albedo 1
    depth[:by, :bx] = 0.0
    albedo[:by, :bx] = 1.0
    m2[-by:, :bx] = (m1[-by:, :bx] * m1[-by:, :bx]) / spp[-by:, :bx].astype(F)   # zero variance
    spp[:by, -bx:] = 1                                      # a single sample
    return dict(color=color, albedo=albedo, normal=normal, depth=depth, moments=np.stack([m1, m2], -1).astype(F), spp=spp)


SETTINGS = dict(iterations=3, demodulate=1, sigma_color=4.0, sigma_depth=1.0)


def test_zero_iterations_is_the_input():
    d = synthetic(17, 13, 1)
    out = denoise_ref(d["color"], d["albedo"], d["normal"], d["depth"], d["moments"], d["spp"],
                      **{**SETTINGS, "iterations": 0})
    assert np.array_equal(out.view(np.uint32), d["color"].view(np.uint32))


@pytest.mark.parametrize("demodulate", [0, 1])
def test_a_constant_image_stays_constant(demodulate):
    d = synthetic(17, 13, 2)
    color = np.broadcast_to(F([0.7, 0.3, 1.9]), d["color"].shape).copy()
    albedo = np.broadcast_to(F([0.5, 0.25, 0.8]), d["color"].shape).copy()
    out = denoise_ref(color, albedo, d["normal"], d["depth"], d["moments"], d["spp"],
                      **{**SETTINGS, "iterations": 5, "demodulate": demodulate})
    assert np.all(np.abs(out - color) <= 1e-6 * color)


def test_orthogonal_half_planes_do_not_mix():
    ny, nx = 12, 20
    color = np.zeros((ny, nx, 3), F)
    normal = np.zeros((ny, nx, 3), F)
    color[:, :10], color[:, 10:] = F([1.0, 0.2, 0.1]), F([0.1, 0.3, 2.0])
    normal[:, :10], normal[:, 10:] = F([1, 0, 0]), F([0, 1, 0])
    albedo = np.ones((ny, nx, 3), F)
    depth = np.full((ny, nx), 4, F)
    out = denoise_ref(color, albedo, normal, depth, **{**SETTINGS, "iterations": 5, "demodulate": 0})
    assert np.array_equal(out.view(np.uint32), color.view(np.uint32))
    # ... while inside a half plane a perturbed pixel is smoothed
    color[5, 4] = F([3, 3, 3])
    out = denoise_ref(color, albedo, normal, depth, **{**SETTINGS, "iterations": 2, "demodulate": 0})
    assert out[5, 4, 0] < 2.5 and np.array_equal(out[:, 10:].view(np.uint32), color[:, 10:].view(np.uint32))


def test_an_all_miss_image_is_returned_unchanged():
    rng = np.random.default_rng(3)
    ny, nx = 9, 17
    color = (rng.random((ny, nx, 3)) * 2).astype(F)
    mom = (rng.random((ny, nx, 2)) * 9).astype(F)
    out = denoise_ref(color, np.ones((ny, nx, 3), F), np.zeros((ny, nx, 3), F), np.zeros((ny, nx), F), mom, 8,
                      **{**SETTINGS, "iterations": 5})
    assert np.array_equal(out.view(np.uint32), color.view(np.uint32))


def test_step_16_on_a_13_wide_image_uses_only_in_image_taps():
    d = synthetic(13, 40, 4)
    _, e, v = prepare_ref(d["color"], d["albedo"], d["moments"], d["spp"], 1)
    e1, v1 = atrous_ref(d["normal"], d["depth"], e, v, 16, 4.0, 1.0, True)
    assert np.isfinite(e1).all() and np.isfinite(v1).all()
    # no tap reaches another column: each column is filtered on its own
    for x in (0, 6, 12):
        ec, vc = atrous_ref(d["normal"][:, x:x + 1], d["depth"][:, x:x + 1], e[:, x:x + 1], v[:, x:x + 1], 16, 4.0, 1.0,
                            True)
        assert np.array_equal(ec.view(np.uint32), e1[:, x:x + 1].view(np.uint32))
        assert np.array_equal(vc.view(np.uint32), v1[:, x:x + 1].view(np.uint32))
    # and on 13 x 13 no tap but the centre is inside: the colour is kept
    e2, _ = atrous_ref(d["normal"][:13], d["depth"][:13], e[:13], v[:13], 16, 4.0, 1.0, True)
    assert np.array_equal(e2.view(np.uint32), e[:13].view(np.uint32))


def test_variance_guidance_stops_at_significant_differences():
    # two flat regions, same guides: a 10-sigma step survives, noise within a region is smoothed
    rng = np.random.default_rng(5)
    ny, nx, N = 16, 32, 8
    mean = np.where(np.arange(nx) < 16, 1.0, 2.0)[None, :, None] * np.ones((ny, 1, 3))
    sigma = 0.1 * np.sqrt(N)                      # per-sample deviation: the mean's is 0.1 per channel
    samples = mean[None] + rng.standard_normal((N, ny, nx, 3)) * sigma
    y = samples.sum(-1).astype(F)
    color = samples.mean(0).astype(F)
    mom = np.stack([y.sum(0), (y * y).sum(0)], -1).astype(F)
    flat = dict(albedo=np.ones((ny, nx, 3), F), normal=np.broadcast_to(F([0, 0, 1]), (ny, nx, 3)).copy(),
                depth=np.full((ny, nx), 3, F))
    out = denoise_ref(color, flat["albedo"], flat["normal"], flat["depth"], mom, N, **{**SETTINGS, "iterations": 4})
    assert np.std(out[:, :12, 0]) < 0.5 * np.std(color[:, :12, 0])
    assert abs(out[:, :12].mean() - 1.0) < 0.05 and abs(out[:, 20:].mean() - 2.0) < 0.05


# ------------------------------------------------------------------ the ABI
def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_ctypes_struct_has_the_headers_layout():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct rt_denoise_params \{(.*?)\} rt_denoise_params;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(typ, n.strip()) for n in names.split(",")]
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    want = []
    for typ, name in fields:
        m = re.fullmatch(r"(\w+)\[(\d+)\]", name)
        want.append((m.group(1), ctype[typ] * int(m.group(2))) if m else (name, ctype[typ]))
    assert [(n, t) for n, t in rtnw.RtDenoiseParams._fields_] == want
    assert ctypes.sizeof(rtnw.RtDenoiseParams) == 32


def test_library_exports_the_denoise_entry_points():
    L = rtnw.lib()
    for name in ("rt_denoise", "rt_denoise_dev", "rt_launch_denoise_prepare", "rt_launch_denoise_atrous"):
        assert hasattr(L, name), name
    assert {"rt_denoise", "rt_denoise_dev"} <= set(rtnw.header_symbols())
    assert L.rt_denoise.argtypes is not None and L.rt_denoise_dev.argtypes is not None


# ------------------------------------------------------------------ argument checks, no GPU
def _call(dp, *, nx=4, ny=3, null=None, moments=True, spp=True, dev=False):
    L = rtnw.lib()
    buf = {k: np.zeros((ny if ny > 0 else 1, nx if nx > 0 else 1, c), np.float32)
           for k, c in (("color", 3), ("albedo", 3), ("normal", 3), ("depth", 1), ("moments", 2), ("out", 3))}
    smap = np.full((max(ny, 1), max(nx, 1)), 4, np.int32)
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in buf.items()}
    mom = ptr["moments"] if moments else None
    sp = smap.ctypes.data if spp else None
    dpp = None if null == "params" else ctypes.byref(dp)
    if dev:   # the pointers are never read on the host
        guides = None if null in ("albedo", "normal", "depth") else ptr["albedo"]
        rc = L.rt_denoise_dev(0, nx, ny, ptr["color"], guides, mom, sp, dpp, ptr["out"], None)
    else:
        rc = L.rt_denoise(0, nx, ny, ptr["color"], ptr["albedo"], ptr["normal"], ptr["depth"], mom, sp, dpp, ptr["out"], None)
    return rc, L.rt_last_error().decode()


def _good(**kw):
    return rtnw.denoise_params(**{**dict(iterations=3, demodulate=1, sigma_color=4.0, sigma_depth=1.0, uniform_spp=0), **kw})


HAVE_DEVICE = rtnw.device_count() > 0
# rt_denoise_dev launches kernels on the pointers it is given: with a device present, arguments
# that pass its checks must come with device memory (tests/test_gpu_denoise.py does that)
DEV_WITHOUT_GPU = pytest.param(True, marks=pytest.mark.skipif(HAVE_DEVICE, reason="a GPU is present"))


def _assert_reaches_the_device(rc, msg):
    if HAVE_DEVICE:   # rt_denoise stages its host buffers itself: a legal call
        assert rc == rtnw.RT_OK, (rc, msg)
    else:             # nothing about the arguments
        assert rc == RT_ERR_HIP, (rc, msg)
        assert "hipSetDevice" in msg, msg


@pytest.mark.parametrize("dev", [False, DEV_WITHOUT_GPU])
def test_valid_arguments_reach_the_device_check(dev):
    for dp, kw in ((_good(), {}), (_good(iterations=0), {}), (_good(iterations=8), {}), (_good(sigma_color=0.0), {}),
                   (_good(uniform_spp=4), dict(spp=False)), (_good(), dict(moments=False, spp=False)),
                   (_good(sigma_depth=float("inf")), {})):
        _assert_reaches_the_device(*_call(dp, dev=dev, **kw))


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("null", ["color", "albedo", "normal", "depth", "out", "params"])
def test_null_arguments_are_invalid(null, dev):
    rc, msg = _call(_good(), null=null, dev=dev)
    assert rc == RT_ERR_INVALID and "null argument" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value,word", [
    ("iterations", -1, "iterations"), ("iterations", 9, "iterations"),
    ("sigma_color", -0.5, "sigma_color"), ("sigma_color", float("nan"), "sigma_color"),
    ("sigma_depth", -1.0, "sigma_depth"), ("sigma_depth", float("nan"), "sigma_depth"),
])
def test_bad_parameters_are_invalid(field, value, word, dev):
    rc, msg = _call(_good(**{field: value}), dev=dev)
    assert rc == RT_ERR_INVALID and word in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("nx,ny", [(0, 3), (4, 0), (-1, 3), (4, -2)])
def test_empty_images_are_invalid(nx, ny, dev):
    rc, msg = _call(_good(), nx=nx, ny=ny, dev=dev)
    assert rc == RT_ERR_INVALID and "nx and ny" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", [0, -4])
def test_moments_without_a_sample_count_are_invalid(n, dev):
    rc, msg = _call(_good(uniform_spp=n), spp=False, dev=dev)
    assert rc == RT_ERR_INVALID and "uniform_spp" in msg, msg
    # without moments the count is not read
    if dev and HAVE_DEVICE:
        return   # a valid call: not with host pointers where a device would read them
    rc, msg = _call(_good(uniform_spp=n), spp=False, moments=False, dev=dev)
    assert rc == (rtnw.RT_OK if HAVE_DEVICE else RT_ERR_HIP), (rc, msg)
