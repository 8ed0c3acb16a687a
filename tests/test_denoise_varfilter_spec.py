"""The denoiser's variance pre-filter (rt_denoise_params.variance_filter), the CPU side: the
exact statement in numpy float32, and the ABI.

With variance_filter = 1 and moments present, the luminance weight's denominator of every
iteration takes a 3 x 3 Gaussian of that iteration's input variance in place of the centre's
own (Schied et al. 2017):

    vbar(p) = sum over dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner), starting from 0.0f,
              of (g[dy] * g[dx]) * v(q'),      g = (0.25, 0.5, 0.25)
    q' = (x + dx, y + dy) if inside the image, else p    (the direct neighbours, not `step` apart)
    lden = sc2 * vbar + 1e-8f

The products g * g are powers of two, so only the nine adds round.  Everything else is
tests/test_denoise_spec.py's filter: the weights, the variance propagated from the unfiltered
v, the e(p) + sum(w (e(q) - e(p))) / sum(w) form and the remodulation.
tests/test_gpu_denoise_varfilter.py compares the GPU's result with `denoise_vf_ref` bit for bit.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rtnw
from conftest import ROOT
from test_denoise_spec import H, denoise_ref, prepare_ref, synthetic

RT_ERR_INVALID = -1
RT_ERR_HIP = -2
F = np.float32
G3 = np.array([0.25, 0.5, 0.25], np.float32)


# ------------------------------------------------------------------ the filter, in numpy
def variance_prefilter(v):
    """vbar: the 3 x 3 Gaussian of v, a neighbour outside the image replaced by the centre."""
    ny, nx = v.shape
    Y, X = np.mgrid[0:ny, 0:nx]
    vbar = np.zeros((ny, nx), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qx, qy = X + dx, Y + dy
            inside = (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
            qx, qy = np.where(inside, qx, X), np.where(inside, qy, Y)
            vbar = vbar + (G3[dy + 1] * G3[dx + 1]) * v[qy, qx]
    assert vbar.dtype == F
    return vbar


def atrous_vf_ref(n, z, e, v, step, sigma_color, sigma_depth, use_var, variance_filter):
    """One iteration with taps `step` apart: (e', v').  test_denoise_spec.atrous_ref with the
    luminance weight's denominator from vbar when use_var and variance_filter."""
    ny, nx = z.shape
    Y, X = np.mgrid[0:ny, 0:nx]
    sc2 = F(sigma_color) * F(sigma_color)
    sz = F(sigma_depth) * F(step)
    lp = (e[..., 0] + e[..., 1]) + e[..., 2]
    lden = sc2 * (variance_prefilter(v) if use_var and variance_filter else v) + F(1e-8)
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
            sv = sv + (w * w) * vq   # the unfiltered variance goes on
    assert sw.dtype == se.dtype == sv.dtype == F
    return e + se / sw[..., None], sv / (sw * sw)


def denoise_vf_ref(color, albedo, normal, depth, moments=None, spp=None, *, iterations, demodulate, sigma_color,
                   sigma_depth, variance_filter=0):
    """rt_denoise with rt_denoise_params.variance_filter on host arrays, bit for bit."""
    color = np.ascontiguousarray(color, F)
    if iterations == 0:
        return color.copy()
    n, z = np.asarray(normal, F), np.asarray(depth, F)
    a, e, v = prepare_ref(color, albedo, moments, spp, demodulate)
    with np.errstate(under="ignore"):
        for i in range(iterations):
            e, v = atrous_vf_ref(n, z, e, v, 1 << i, sigma_color, sigma_depth, moments is not None, variance_filter)
    return e * a


SETTINGS = dict(iterations=3, demodulate=1, sigma_color=4.0, sigma_depth=1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(d, vf, moments=True, **kw):
    mom, spp = (d["moments"], d["spp"]) if moments else (None, None)
    return denoise_vf_ref(d["color"], d["albedo"], d["normal"], d["depth"], mom, spp, **{**SETTINGS, **kw},
                          variance_filter=vf)


def test_prefilter_on_hand_cases():
    # a constant plane stays constant, edges included (the centre stands in for what is outside)
    assert np.array_equal(variance_prefilter(np.full((4, 5), 3.0, F)), np.full((4, 5), 3.0, F))
    # one unit spike spreads as the 1 2 1 / 4 kernel's outer product
    v = np.zeros((5, 5), F)
    v[2, 2] = 1.0
    assert np.array_equal(variance_prefilter(v)[1:4, 1:4], np.outer(G3, G3))
    # a 1 x 1 image: nine times the centre, summing to it (0.75: every partial sum is exact)
    assert variance_prefilter(np.full((1, 1), 0.75, F))[0, 0] == F(0.75)
    # a corner: the five outside cells take the corner's own value
    v = np.arange(12, dtype=F).reshape(3, 4)
    want = F(0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inside = 0 <= dy and 0 <= dx
            want = want + (G3[dy + 1] * G3[dx + 1]) * (v[dy, dx] if inside else v[0, 0])
    assert variance_prefilter(v)[0, 0] == want


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
def test_variance_filter_0_is_the_filter_of_before(seed, iterations):
    d = synthetic(33, 40, seed)
    got = _run(d, 0, iterations=iterations)
    want = denoise_ref(d["color"], d["albedo"], d["normal"], d["depth"], d["moments"], d["spp"],
                       **{**SETTINGS, "iterations": iterations})
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_variance_filter_1_differs_and_opens_the_one_sample_block(seed):
    nx, ny = 33, 40
    d = synthetic(nx, ny, seed)
    off, on = _run(d, 0), _run(d, 1)
    assert np.isfinite(on).all()
    assert not np.array_equal(bits(off), bits(on))
    # the spp = 1 block (top right): v = 0 there and lden = 1e-8 before, so a tap whose luminance
    # differs at all was rejected; one iteration shows it
    by, bx = max(1, ny // 3), max(1, nx // 3)
    off1, on1 = _run(d, 0, iterations=1), _run(d, 1, iterations=1)
    blk = (slice(0, by), slice(nx - bx, nx))
    assert (d["spp"][blk] == 1).all()
    assert not np.array_equal(bits(off1[blk]), bits(on1[blk]))
    # its interior (every direct neighbour has v = 0 too) keeps lden = 1e-8 in the first iteration
    inner = (slice(0, by - 1), slice(nx - bx + 1, nx))
    assert np.array_equal(bits(off1[inner]), bits(on1[inner]))


@pytest.mark.parametrize("iterations", [1, 3])
def test_without_moments_the_switch_has_no_effect(iterations):
    d = synthetic(33, 40, 4)
    assert np.array_equal(bits(_run(d, 0, moments=False, iterations=iterations)),
                          bits(_run(d, 1, moments=False, iterations=iterations)))


# ------------------------------------------------------------------ the ABI
def test_struct_layout_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct rt_denoise_params \{(.*?)\} rt_denoise_params;", text, flags=re.S).group(1)
    decls = [" ".join(x.split()) for x in body.split(";") if x.strip()]
    assert decls[-2:] == ["int32_t variance_filter", "int32_t pad[2]"], decls
    names = [n for n, _ in rtnw.RtDenoiseParams._fields_]
    assert names == ["iterations", "demodulate", "sigma_color", "sigma_depth", "uniform_spp", "variance_filter", "pad"]
    assert ctypes.sizeof(rtnw.RtDenoiseParams) == 32
    assert rtnw.RtDenoiseParams.variance_filter.offset == 20 and rtnw.RtDenoiseParams.variance_filter.size == 4
    assert rtnw.denoise_params().variance_filter == 0              # every existing caller gets 0
    assert rtnw.denoise_params(variance_filter=1).variance_filter == 1
    assert "variance_filter" not in rtnw.DENOISE_DEFAULTS


def _call(dp, *, dev, moments=True):
    L = rtnw.lib()
    nx, ny = 4, 3
    buf = {k: np.zeros((ny, nx, c), np.float32)
           for k, c in (("color", 3), ("albedo", 3), ("normal", 3), ("depth", 1), ("moments", 2), ("out", 3))}
    smap = np.full((ny, nx), 4, np.int32)
    mom = buf["moments"].ctypes.data if moments else None
    sp = smap.ctypes.data if moments else None
    if dev:   # the pointers are never read on the host
        rc = L.rt_denoise_dev(0, nx, ny, buf["color"].ctypes.data, buf["albedo"].ctypes.data, mom, sp, ctypes.byref(dp),
                              buf["out"].ctypes.data, None)
    else:
        rc = L.rt_denoise(0, nx, ny, buf["color"].ctypes.data, buf["albedo"].ctypes.data, buf["normal"].ctypes.data,
                          buf["depth"].ctypes.data, mom, sp, ctypes.byref(dp), buf["out"].ctypes.data, None)
    return rc, L.rt_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("value", [2, -1])
@pytest.mark.parametrize("moments", [True, False])
def test_a_variance_filter_other_than_0_or_1_is_invalid(value, dev, moments):
    rc, msg = _call(rtnw.denoise_params(variance_filter=value, **SETTINGS), dev=dev, moments=moments)
    assert rc == RT_ERR_INVALID and "variance_filter" in msg, msg


@pytest.mark.parametrize("value", [0, 1])
def test_0_and_1_pass_the_argument_checks(value):
    # the host entry point with host buffers: on to the device (RT_ERR_HIP where there is none)
    rc, msg = _call(rtnw.denoise_params(variance_filter=value, **SETTINGS), dev=False)
    assert rc != RT_ERR_INVALID, (rc, msg)
