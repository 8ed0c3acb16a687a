"""The firefly clamp, the CPU side: the exact statement of the rule, the ABI's struct and entry
points, the argument checks of rt_firefly / rt_firefly_dev (made before any HIP call, so they
answer without a GPU), and the rule on the oracle's cornell_box.

The rule is stated here in numpy float32, not in the product:
tests/test_gpu_firefly.py imports `firefly_ref` and compares the GPU's result with it bit for
bit.  Every operation is an add, subtract, multiply, IEEE divide, max, min, abs or comparison on
float32 values, in the order written; rt_firefly.hip performs the same sequence without
contraction.  For pixel p, with r = radius:

    a' = demodulate ? max(albedo, 0.01f) per channel : (1, 1, 1)      # rt_denoise's floor
    e  = c / a'                          l = (e0 + e1) + e2
    s  = (albedo0 + albedo1) + albedo2   # the raw albedo, whatever demodulate says
    cnt = 0, sum = 0.0f
    for dy = -r..r (outer), dx = -r..r (inner), (dx, dy) != (0, 0), q = (x+dx, y+dy) inside the image:
        dn  = (n_p0*n_q0 + n_p1*n_q1) + n_p2*n_q2
        sim = dn >= cos_normal
              and |z_p - z_q| <= sigma_depth  * min(z_p, z_q) + 1e-6f
              and |s_p - s_q| <= sigma_albedo * min(s_p, s_q) + 1e-6f
        if sim: cnt += 1; sum = sum + l_q
    clamped = cnt >= min_similar and l_p > (bound = k * (sum / float(cnt)) + floor)
    ratio   = clamped ? bound / l_p : 1.0f
    out     = clamped ? (e * ratio) * a' : c             # an untouched pixel is the input bit for bit
    m1'     = clamped ? m1 * ratio : m1 ;  m2' = clamped ? (m2 * ratio) * ratio : m2

A Jacobi pass: every value read is an input; neighbours outside the image do not exist.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle as O
import rtnw
from conftest import ROOT
from test_denoise_spec import ALBEDO_MIN, synthetic

RT_ERR_INVALID = -1
RT_ERR_HIP = -2
F = np.float32
THREADS = min(16, os.cpu_count() or 1)


# ------------------------------------------------------------------ the rule, in numpy
def firefly_ref(color, albedo, normal, depth, moments=None, *, demodulate, radius, min_similar, k, floor, cos_normal,
                sigma_depth, sigma_albedo):
    """rt_firefly on host arrays ([ny, nx, ...] float32), bit for bit: (out, moments' or None, ratio)."""
    c = np.ascontiguousarray(color, F)
    alb, n, z = np.asarray(albedo, F), np.asarray(normal, F), np.asarray(depth, F)
    ny, nx = z.shape
    a = np.maximum(alb, ALBEDO_MIN) if demodulate else np.ones(c.shape, F)
    e = c / a
    l = (e[..., 0] + e[..., 1]) + e[..., 2]
    s = (alb[..., 0] + alb[..., 1]) + alb[..., 2]
    Y, X = np.mgrid[0:ny, 0:nx]
    cnt = np.zeros((ny, nx), np.int32)
    sm = np.zeros((ny, nx), F)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            qx, qy = X + dx, Y + dy
            inside = (qx >= 0) & (qx < nx) & (qy >= 0) & (qy < ny)
            qx, qy = np.where(inside, qx, X), np.where(inside, qy, Y)   # any in-image cell: `inside` masks it
            nq, zq, sq, lq = n[qy, qx], z[qy, qx], s[qy, qx], l[qy, qx]
            dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            sim = inside & (dn >= F(cos_normal)) \
                & (np.abs(z - zq) <= F(sigma_depth) * np.minimum(z, zq) + F(1e-6)) \
                & (np.abs(s - sq) <= F(sigma_albedo) * np.minimum(s, sq) + F(1e-6))
            cnt = cnt + sim
            sm = np.where(sim, sm + lq, sm)
    assert sm.dtype == l.dtype == s.dtype == F
    with np.errstate(all="ignore"):
        bound = F(k) * (sm / cnt.astype(F)) + F(floor)
        clamped = (cnt >= min_similar) & (l > bound)
        ratio = np.where(clamped, bound / l, F(1)).astype(F)
        out = np.where(clamped[..., None], (e * ratio[..., None]) * a, c).astype(F)
    mom = None
    if moments is not None:
        m = np.asarray(moments, F)
        with np.errstate(all="ignore"):
            mom = np.stack([np.where(clamped, m[..., 0] * ratio, m[..., 0]),
                            np.where(clamped, (m[..., 1] * ratio) * ratio, m[..., 1])], -1).astype(F)
    return out, mom, ratio


SETTINGS = dict(demodulate=1, radius=1, min_similar=3, k=4.0, floor=0.01, cos_normal=0.9, sigma_depth=0.1,
                sigma_albedo=0.25)


# looser guides and a lower bar for test_denoise_spec.synthetic, whose neighbours rarely agree: a few per
# cent of its pixels are clamped at these, under SETTINGS none
SYNTHETIC = dict(demodulate=1, radius=1, min_similar=2, k=2.0, floor=0.01, cos_normal=0.5, sigma_depth=0.2,
                 sigma_albedo=0.5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def plane(nx, ny, value=0.5, albedo=(0.5, 0.25, 0.8)):
    """A flat plane facing the camera: every pixel similar to every other."""
    return dict(color=np.full((ny, nx, 3), value, F), albedo=np.broadcast_to(F(albedo), (ny, nx, 3)).copy(),
                normal=np.broadcast_to(F([0, 0, 1]), (ny, nx, 3)).copy(), depth=np.full((ny, nx), 4, F),
                moments=np.stack([np.full((ny, nx), 6.0, F), np.full((ny, nx), 7.5, F)], -1))


def run(d, moments=True, **kw):
    return firefly_ref(d["color"], d["albedo"], d["normal"], d["depth"], d["moments"] if moments else None,
                       **{**SETTINGS, **kw})


@pytest.mark.parametrize("demodulate", [0, 1])
def test_a_spike_on_a_plane_becomes_the_bound_and_nothing_else_changes(demodulate):
    d = plane(9, 7)
    d["color"][3, 4] *= F(50)
    out, mom, ratio = run(d, demodulate=demodulate)
    a = np.maximum(d["albedo"], ALBEDO_MIN) if demodulate else np.ones((7, 9, 3), F)
    e = d["color"] / a
    l = (e[..., 0] + e[..., 1]) + e[..., 2]
    mean = F(0)
    for _ in range(8):
        mean = mean + l[0, 0]
    bound = F(4.0) * (mean / F(8)) + F(0.01)
    r = bound / l[3, 4]
    assert ratio[3, 4] == r and r < 1
    assert np.array_equal(bits(out[3, 4]), bits((e[3, 4] * r) * a[3, 4]))
    lo = (out[3, 4] / a[3, 4]).sum(dtype=np.float64)
    assert abs(lo - float(bound)) <= 1e-6 * float(bound)       # k * mean + floor, but for a few float32 roundings
    keep = np.ones((7, 9), bool)
    keep[3, 4] = False
    assert np.array_equal(bits(out[keep]), bits(d["color"][keep])) and (ratio[keep] == 1).all()
    # the spike's neighbours saw it in their means, and were not clamped for that (Jacobi: inputs only)
    assert np.array_equal(bits(mom[keep]), bits(d["moments"][keep]))
    assert mom[3, 4, 0] == d["moments"][3, 4, 0] * r and mom[3, 4, 1] == (d["moments"][3, 4, 1] * r) * r


def test_fewer_than_min_similar_neighbours_leave_the_pixel_alone():
    d = plane(9, 7)
    d["color"][3, 4] *= F(50)
    d["normal"][2:5, 3:6] = F([1, 0, 0])         # the 3 x 3 around the spike faces elsewhere ...
    d["normal"][3, 4] = F([0, 0, 1])             # ... but for the spike: 0 similar neighbours
    d["normal"][2, 3] = d["normal"][2, 4] = F([0, 0, 1])   # two: still below min_similar = 3
    out, _, ratio = run(d)
    assert np.array_equal(bits(out), bits(d["color"])) and (ratio == 1).all()
    assert run(d, min_similar=2)[2][3, 4] < 1    # with 2 asked for it is clamped


def test_an_emitter_pixel_is_untouched():
    d = plane(9, 7)
    d["color"][3, 4] = F([15, 15, 15])
    d["albedo"][3, 4] = F([15, 15, 15])          # a light's guide albedo is its emission
    for demodulate in (0, 1):
        out, mom, ratio = run(d, demodulate=demodulate)
        assert np.array_equal(bits(out), bits(d["color"])) and (ratio == 1).all()
        assert np.array_equal(bits(mom), bits(d["moments"]))
    # the same radiance with the plane's albedo is a firefly
    d["albedo"][3, 4] = d["albedo"][0, 0]
    assert run(d)[2][3, 4] < 1


def test_a_huge_k_returns_the_input():
    d = synthetic(33, 40, 7)
    d["color"][5, 5] *= F(50)
    assert 20 < (run(d, **SYNTHETIC)[2] < 1).sum() < d["depth"].size // 4
    out, mom, ratio = run(d, **{**SYNTHETIC, "k": 3e38})
    assert np.array_equal(bits(out), bits(d["color"])) and np.array_equal(bits(mom), bits(d["moments"]))
    out, mom, ratio = run(d, k=3e38, cos_normal=-1.0, sigma_depth=1e30, sigma_albedo=1e30)
    assert np.array_equal(bits(out), bits(d["color"])) and np.array_equal(bits(mom), bits(d["moments"]))
    assert (ratio == 1).all()


def test_a_one_pixel_image_is_untouched():
    d = plane(1, 1, value=1e6)
    for r in (1, 2, 3):
        out, mom, ratio = run(d, radius=r, min_similar=1)
        assert np.array_equal(bits(out), bits(d["color"])) and ratio[0, 0] == 1
        assert np.array_equal(bits(mom), bits(d["moments"]))


def test_at_a_corner_only_the_three_inside_neighbours_count():
    d = plane(5, 4)
    d["color"][0, 0] *= F(50)
    assert run(d, min_similar=4)[2][0, 0] == 1          # no centre stands in for the 5 outside
    out, _, ratio = run(d, min_similar=3)
    l = F(0.5) / F(0.5) + F(0.5) / F(0.25) + F(0.5) / F(0.8)
    bound = F(4.0) * (((l + l) + l) / F(3)) + F(0.01)
    assert ratio[0, 0] == bound / (((F(25) / F(0.5)) + (F(25) / F(0.25))) + F(25) / F(0.8))
    # an edge pixel has 5
    d = plane(5, 4)
    d["color"][0, 2] *= F(50)
    assert run(d, min_similar=6)[2][0, 2] == 1 and run(d, min_similar=5)[2][0, 2] < 1


def test_misses_are_similar_only_when_cos_normal_allows_it():
    d = plane(6, 5)
    d["normal"][...] = 0
    d["depth"][...] = 0
    d["albedo"][...] = 1
    d["color"][2, 3] *= F(50)
    assert (run(d, cos_normal=0.9)[2] == 1).all()
    assert (run(d, cos_normal=1e-3)[2] == 1).all()
    assert run(d, cos_normal=0.0)[2][2, 3] < 1


def test_moments_follow_the_ratio_and_are_optional():
    d = synthetic(33, 40, 8)
    d["color"][7, 9] *= F(50)
    out, mom, ratio = run(d, **SYNTHETIC)
    out2, none, ratio2 = run(d, moments=False, **SYNTHETIC)
    assert none is None and np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(ratio), bits(ratio2))
    c = ratio != 1
    assert c.any() and not c.all()
    m = d["moments"]
    assert np.array_equal(bits(mom[~c]), bits(m[~c]))
    assert np.array_equal(bits(mom[c][:, 0]), bits(m[c][:, 0] * ratio[c]))
    assert np.array_equal(bits(mom[c][:, 1]), bits((m[c][:, 1] * ratio[c]) * ratio[c]))


# ------------------------------------------------------------------ the ABI
def test_ctypes_struct_has_the_headers_layout():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct rt_firefly_params \{(.*?)\} rt_firefly_params;", text, flags=re.S).group(1)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    want = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.strip().split(None, 1)
            want += [(n.strip(), ctype[typ]) for n in names.split(",")]
    assert [(n, t) for n, t in rtnw.RtFireflyParams._fields_] == want
    assert ctypes.sizeof(rtnw.RtFireflyParams) == 32
    assert set(rtnw.FIREFLY_DEFAULTS) == {n for n, _ in want}
    fp = rtnw.firefly_params()
    assert all(getattr(fp, n) == ctype_value(rtnw.FIREFLY_DEFAULTS[n], t) for n, t in want)


def ctype_value(v, t):
    return t(v).value


def test_library_exports_the_firefly_entry_points():
    L = rtnw.lib()
    for name in ("rt_firefly", "rt_firefly_dev", "rt_launch_firefly"):
        assert hasattr(L, name), name
    assert {"rt_firefly", "rt_firefly_dev"} <= set(rtnw.header_symbols())
    assert L.rt_firefly.argtypes is not None and L.rt_firefly_dev.argtypes is not None
    assert hasattr(rtnw, "firefly") and hasattr(rtnw, "firefly_params")


# ------------------------------------------------------------------ argument checks, no GPU
def _call(fp, *, nx=4, ny=3, null=None, moments=True, out_moments=True, ratio=True, in_place=False, dev=False):
    L = rtnw.lib()
    h, w = max(ny, 1), max(nx, 1)
    buf = {k: np.zeros((h, w, c), np.float32)
           for k, c in (("color", 3), ("albedo", 3), ("normal", 3), ("depth", 1), ("moments", 2), ("out", 3),
                        ("out_moments", 2), ("ratio", 1))}
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in buf.items()}
    mom = ptr["moments"] if moments else None
    om = ptr["out_moments"] if out_moments else None
    rt = ptr["ratio"] if ratio else None
    out = ptr["color"] if in_place else ptr["out"]
    fpp = None if null == "params" else ctypes.byref(fp)
    if dev:   # the pointers are never read on the host
        guides = None if null in ("albedo", "normal", "depth") else ptr["albedo"]
        rc = L.rt_firefly_dev(0, nx, ny, ptr["color"], guides, mom, fpp, out, om, rt, None)
    else:
        rc = L.rt_firefly(0, nx, ny, ptr["color"], ptr["albedo"], ptr["normal"], ptr["depth"], mom, fpp, out, om, rt, None)
    return rc, L.rt_last_error().decode()


def _good(**kw):
    return rtnw.firefly_params(**{**SETTINGS, **kw})


HAVE_DEVICE = rtnw.device_count() > 0
# rt_firefly_dev launches a kernel on the pointers it is given: with a device present, arguments
# that pass its checks must come with device memory (tests/test_gpu_firefly.py does that)
DEV_WITHOUT_GPU = pytest.param(True, marks=pytest.mark.skipif(HAVE_DEVICE, reason="a GPU is present"))


@pytest.mark.parametrize("dev", [False, DEV_WITHOUT_GPU])
def test_valid_arguments_reach_the_device_check(dev):
    inf = float("inf")
    for fp, kw in ((_good(), {}), (_good(demodulate=0), {}), (_good(radius=3, min_similar=48), {}),
                   (_good(radius=2, min_similar=24), {}), (_good(min_similar=8), {}), (_good(k=1.0), {}), (_good(k=inf), {}),
                   (_good(floor=0.0), {}), (_good(cos_normal=-1.0), {}), (_good(cos_normal=1.0), {}),
                   (_good(sigma_depth=0.0, sigma_albedo=0.0), {}), (_good(sigma_depth=inf, sigma_albedo=inf), {}),
                   (_good(), dict(moments=False, out_moments=False)), (_good(), dict(out_moments=False, ratio=False))):
        rc, msg = _call(fp, dev=dev, **kw)
        assert rc != RT_ERR_INVALID, (rc, msg)
        if HAVE_DEVICE:   # rt_firefly stages its host buffers itself: a legal call
            assert rc == rtnw.RT_OK, (rc, msg)
        else:             # nothing about the arguments
            assert rc == RT_ERR_HIP and "hipSetDevice" in msg, (rc, msg)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("null", ["color", "albedo", "normal", "depth", "out", "params"])
def test_null_arguments_are_invalid(null, dev):
    rc, msg = _call(_good(), null=null, dev=dev)
    assert rc == RT_ERR_INVALID and "null argument" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [
    ("demodulate", 2), ("demodulate", -1), ("radius", 0), ("radius", 4), ("radius", -1),
    ("min_similar", 0), ("min_similar", 9), ("min_similar", -3),
    ("k", 0.5), ("k", -2.0), ("k", float("nan")),
    ("floor", -0.01), ("floor", float("inf")), ("floor", float("nan")),
    ("cos_normal", -1.5), ("cos_normal", 1.01), ("cos_normal", float("nan")),
    ("sigma_depth", -1.0), ("sigma_depth", float("nan")), ("sigma_albedo", -0.5), ("sigma_albedo", float("nan")),
])
def test_bad_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(**{field: value}), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("radius,most", [(1, 8), (2, 24), (3, 48)])
def test_min_similar_is_bounded_by_the_window(radius, most, dev):
    rc, msg = _call(_good(radius=radius, min_similar=most + 1), dev=dev)
    assert rc == RT_ERR_INVALID and "min_similar" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("nx,ny", [(0, 3), (4, 0), (-1, 3), (4, -2), (65536, 32768), (1 << 30, 2)])
def test_empty_and_oversized_images_are_invalid(nx, ny, dev):
    L = rtnw.lib()
    one = np.zeros(8, np.float32).ctypes.data      # never read: the size check comes first
    fp = _good()
    if dev:
        rc = L.rt_firefly_dev(0, nx, ny, one, one, None, ctypes.byref(fp), one + 4, None, None, None)
    else:
        rc = L.rt_firefly(0, nx, ny, one, one, one, one, None, ctypes.byref(fp), one + 4, None, None, None)
    msg = L.rt_last_error().decode()
    assert rc == RT_ERR_INVALID and "nx and ny" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
def test_out_moments_without_moments_is_invalid(dev):
    rc, msg = _call(_good(), moments=False, out_moments=True, dev=dev)
    assert rc == RT_ERR_INVALID and "out_moments" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
def test_in_place_is_invalid(dev):
    rc, msg = _call(_good(), in_place=True, dev=dev)
    assert rc == RT_ERR_INVALID and "out" in msg and "color" in msg, msg


# ------------------------------------------------------------------ on the oracle's cornell_box
NX = NY = 48
SPP, SEED = 8, 31
RENDERED = dict(demodulate=1, radius=1, k=4.0, floor=0.01, min_similar=3, cos_normal=0.9, sigma_depth=0.1,
                sigma_albedo=0.25)
_rendered = {}


def oracle_cornell():
    """(colour, guides) of the oracle's cornell_box 48 x 48 at 8 spp, kernel statement; computed once."""
    if not _rendered:
        color, _ = O.render(O.kernel_spec("cornell_box", NX, NY, SPP, seed=SEED, chunk=1, threads=THREADS))
        cam_name, bg, depth = rtnw.SCENE_DEFAULTS["cornell_box"]
        fh = O.first_hits_desc(rtnw.SceneDesc.builtin("cornell_box"), rtnw.Camera.preset(cam_name, NX, NY),
                               O.desc_spec(NX, NY, SPP, max_depth=depth, background="black", seed=SEED, chunk=1,
                                           threads=THREADS))
        f = O.feature_means(fh)
        for v in (color, *f.values()):
            v.setflags(write=False)
        _rendered.update(color=color, f=f)
    return _rendered["color"], _rendered["f"]


def test_the_rule_on_the_oracles_cornell_box_keeps_the_light_and_clamps_fireflies():
    """cornell_box 48 x 48, 8 spp, seed 31: the guided rule clamps 199 of the 2304 pixels (222
    with every neighbour similar), the smallest ratio 0.0013, and none of the 16 pixels of the
    light's interior (coverage 1, guide albedo sum above 3)."""
    color, f = oracle_cornell()
    out, _, ratio = firefly_ref(color, f["albedo"], f["normal"], f["depth"], **RENDERED)
    light = (f["coverage"] == 1) & (f["albedo"].sum(-1) > 3)
    assert light.sum() >= 4, int(light.sum())
    assert np.array_equal(bits(out[light]), bits(color[light])) and (ratio[light] == 1).all()
    clamped = ratio != 1
    unguided, _, r0 = firefly_ref(color, f["albedo"], f["normal"], f["depth"],
                                  **{**RENDERED, "cos_normal": -1.0, "sigma_depth": 1e30, "sigma_albedo": 1e30})
    print(f"cornell_box {NX}x{NY} at {SPP} spp, seed {SEED}: {int(clamped.sum())} of {clamped.size} pixels clamped, "
          f"{int((r0 != 1).sum())} without the guides, {int(light.sum())} light pixels, "
          f"smallest ratio {float(ratio.min()):.4f}")
    assert clamped.sum() >= 1
    assert (ratio[clamped] < 1).all() and (ratio[clamped] > 0).all()
    assert np.array_equal(bits(out[~clamped]), bits(color[~clamped]))
    lum = lambda img: img.sum(-1)
    assert (lum(out)[clamped] < lum(color)[clamped]).all()
