"""Adaptive sampling, the CPU side: the ABI's new structs, the argument checks of
rt_render_adaptive and rt_render_tiles_moments (made before any HIP call, so they answer
without a GPU), and the convergence rule.

The rule is stated here in numpy float64, not in the product: tests/test_gpu_adaptive.py
imports `converged` and `spp_schedule` to predict the GPU's sample-count map.  The
implementation's behaviour for tolerance <= 0 is "never": checked before the formula, so a
pixel of zero variance (lhs = 0 <= rhs = 0) does not converge either.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rtnw
from conftest import ROOT

RT_ERR_INVALID = -1


# ------------------------------------------------------------------ the rule, in numpy
def converged(n, m1, m2, tol, floor):
    """include/rt_hip.h rt_render_adaptive: FP64, multiplies / adds / subtracts in this order.
    n: samples so far; m1, m2: float32 sums of y and y*y; tol, floor: float32 parameters."""
    m1 = np.asarray(m1, np.float32)
    m2 = np.asarray(m2, np.float32)
    tol = np.float32(tol)
    if not tol > 0:                      # "never", before the formula
        return np.zeros(np.broadcast(m1, m2).shape, bool)
    N = np.float64(n)
    S1 = m1.astype(np.float64)
    S2 = m2.astype(np.float64)
    with np.errstate(all="ignore"):
        lhs = N * S2 - S1 * S1
        t = S1 + np.float64(np.float32(floor)) * N
        rhs = ((np.float64(tol) * np.float64(tol)) * (N - 1.0)) * (t * t)
        return lhs <= rhs                # NaN compares false


def spp_schedule(min_spp, step_spp, cap):
    """Sample counts after each pass: min_spp, then + step_spp, the last clipped to cap."""
    out = [min_spp]
    while out[-1] < cap:
        out.append(min(out[-1] + step_spp, cap))
    return out


def moments_f32(ys):
    """float32 running sums of y and y*y over the leading axis, in order, no FMA."""
    ys = np.asarray(ys, np.float32)
    m1 = np.zeros(ys.shape[1:], np.float32)
    m2 = np.zeros(ys.shape[1:], np.float32)
    for y in ys:
        m1 = (m1 + y).astype(np.float32)
        m2 = (m2 + (y * y).astype(np.float32)).astype(np.float32)
    return m1, m2


def test_rule_on_hand_cases():
    # zero variance: four equal samples y = 0.5 -> lhs = 4 * 1 - 2 * 2 = 0 <= rhs
    m1, m2 = moments_f32([[0.5]] * 4)
    assert m1[0] == 2.0 and m2[0] == 1.0
    assert converged(4, m1, m2, 0.1, 0.0).all()
    assert converged(4, m1, m2, 1e-6, 0.0).all()
    # a black pixel converges with any floor, and with none (0 <= 0)
    assert converged(4, [0.0], [0.0], 0.1, 0.01).all() and converged(4, [0.0], [0.0], 0.1, 0.0).all()
    # tolerance <= 0: never, the zero-variance pixel (lhs <= 0) included
    for tol in (0.0, -1.0, -np.inf):
        assert not converged(4, m1, m2, tol, 0.0).any()
        assert not converged(4, [0.0], [0.0], tol, 0.01).any()
    # y = 0, 1, 0, 1: mean 0.5, sample variance 1/3, SEM = sqrt(1/12) = 0.2887: relative 0.577
    m1, m2 = moments_f32([[0.0], [1.0], [0.0], [1.0]])
    assert m1[0] == 2.0 and m2[0] == 2.0
    assert not converged(4, m1, m2, 0.57, 0.0).any()
    assert converged(4, m1, m2, 0.58, 0.0).all()
    # lhs = 4 * 2 - 4 = 4; rhs = tol^2 * 3 * (2 + 4 floor)^2: floor 0.5 -> tol^2 * 48 >= 4 from tol = 0.2887
    assert not converged(4, m1, m2, 0.28, 0.5).any()
    assert converged(4, m1, m2, 0.29, 0.5).all()
    # a NaN or infinite moment does not converge (inf - inf and inf <= inf * ... aside: NaN compares false)
    nan = np.float32(np.nan)
    assert not converged(4, [nan], [1.0], 0.5, 0.01).any()
    assert not converged(4, [1.0], [nan], 0.5, 0.01).any()
    assert not converged(4, [nan], [nan], np.inf, 0.01).any()
    assert not converged(4, [np.inf], [np.inf], 0.5, 0.01).any()
    # elementwise over a map
    got = converged(4, np.float32([2, 2, 0]), np.float32([1, 2, 0]), 0.3, 0.0)
    assert got.tolist() == [True, False, True]


def test_schedule():
    assert spp_schedule(4, 4, 16) == [4, 8, 12, 16]
    assert spp_schedule(2, 3, 9) == [2, 5, 8, 9]
    assert spp_schedule(16, 1, 16) == [16]


# ------------------------------------------------------------------ the ABI's structs
def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def _struct_fields(name):
    """(type, field) pairs of `typedef struct name { ... } name;` in the header."""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_ctypes_structs_have_the_headers_layout():
    size = {"int32_t": 4, "float": 4, "double": 8}
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}
    for name, cls in (("rt_adaptive_params", rtnw.RtAdaptiveParams), ("rt_adaptive_stats", rtnw.RtAdaptiveStats)):
        fields = _struct_fields(name)
        assert [(n, t) for n, t in cls._fields_] == [(n, ctype[t]) for t, n in fields], name
        assert ctypes.sizeof(cls) == sum(size[t] for t, _ in fields), name   # no padding: equal-sized members
    assert ctypes.sizeof(rtnw.RtAdaptiveParams) == 16
    assert ctypes.sizeof(rtnw.RtAdaptiveStats) == 56
    assert re.search(r"#define RT_ABI_VERSION 2\b", _header())


def test_library_exports_the_new_entry_points():
    L = rtnw.lib()
    for name in ("rt_render_tiles_moments", "rt_render_adaptive", "rt_copy_to_device", "rt_launch_resolve_moments",
                 "rt_launch_adaptive_select", "rt_launch_adaptive_finish"):
        assert hasattr(L, name), name
    assert {"rt_render_tiles_moments", "rt_render_adaptive"} <= set(rtnw.header_symbols())


# ------------------------------------------------------------------ argument checks, no GPU
def _adaptive(params, ap, *, scene=None, cam=True, out=True, p=True, a=True):
    """rt_render_adaptive with a null scene: every argument check comes before any HIP call,
    the scene's last, so each bad value is reported by name without a device."""
    L = rtnw.lib()
    camd = rtnw.RtCameraDesc()
    buf = np.zeros((2, 2, 3), np.float32)
    rc = L.rt_render_adaptive(scene, ctypes.byref(camd) if cam else None, ctypes.byref(params) if p else None,
                              ctypes.byref(ap) if a else None, 0, 0, 2, 2, buf.ctypes.data if out else None, None, None,
                              None)
    return rc, L.rt_last_error().decode()


def _good():
    return (rtnw.RenderParams(2, 2, 16, seed=1),
            rtnw.RtAdaptiveParams(min_spp=4, step_spp=4, tolerance=0.25, floor=0.01))


def test_valid_arguments_reach_the_scene_check():
    rc, msg = _adaptive(*_good())
    assert rc == RT_ERR_INVALID and "null scene" in msg, msg
    # RT_FLAG_RIGHT_FOLD passes the argument checks; so do tolerance <= 0 and +inf, floor 0, min_spp == cap
    p, a = _good()
    p.flags = rtnw.RT_FLAG_RIGHT_FOLD
    a.tolerance, a.floor, a.min_spp = 0.0, 0.0, 16
    assert "null scene" in _adaptive(p, a)[1]
    a.tolerance = float("inf")
    assert "null scene" in _adaptive(p, a)[1]
    a.tolerance = -1.0
    assert "null scene" in _adaptive(p, a)[1]


@pytest.mark.parametrize("null", ["cam", "p", "a", "out"])
def test_null_arguments_are_invalid(null):
    rc, msg = _adaptive(*_good(), **{null: False})
    assert rc == RT_ERR_INVALID and "null argument" in msg, msg


@pytest.mark.parametrize("field,value,word", [
    ("min_spp", 1, "min_spp"), ("min_spp", 0, "min_spp"), ("min_spp", -3, "min_spp"),
    ("step_spp", 0, "step_spp"), ("step_spp", -1, "step_spp"),
    ("min_spp", 17, "cap"),                       # p->spp < min_spp
    ("floor", -0.5, "floor"), ("floor", float("inf"), "floor"), ("floor", float("nan"), "floor"),
    ("tolerance", float("nan"), "tolerance"),
])
def test_bad_adaptive_parameters_are_invalid(field, value, word):
    p, a = _good()
    setattr(a, field, value)
    rc, msg = _adaptive(p, a)
    assert rc == RT_ERR_INVALID and word in msg, msg


@pytest.mark.parametrize("flag", ["RT_FLAG_COUNT", "RT_FLAG_PROFILE", "RT_FLAG_SUM_IN", "RT_FLAG_SUM_OUT"])
def test_unsupported_flags_are_invalid(flag):
    p, a = _good()
    p.flags = getattr(rtnw, flag) | rtnw.RT_FLAG_RIGHT_FOLD
    rc, msg = _adaptive(p, a)
    assert rc == RT_ERR_INVALID and flag in msg and "null scene" not in msg, msg


def test_sample_offset_is_invalid():
    p, a = _good()
    p.sample_offset = 4
    rc, msg = _adaptive(p, a)
    assert rc == RT_ERR_INVALID and "sample_offset" in msg, msg


@pytest.mark.parametrize("flag", ["RT_FLAG_COUNT", "RT_FLAG_PROFILE"])
def test_tiles_moments_rejects_count_and_profile(flag):
    L = rtnw.lib()
    p = rtnw.RenderParams(2, 2, 4, flags=getattr(rtnw, flag))
    camd = rtnw.RtCameraDesc()
    tile = (ctypes.c_int32 * 4)(0, 0, 2, 2)
    rc = L.rt_render_tiles_moments(None, ctypes.byref(camd), ctypes.byref(p), tile, 1, None, None, None, None)
    msg = L.rt_last_error().decode()
    assert rc == RT_ERR_INVALID and flag in msg, msg
    p.flags = 0
    rc = L.rt_render_tiles_moments(None, ctypes.byref(camd), ctypes.byref(p), tile, 1, None, None, None, None)
    assert rc == RT_ERR_INVALID and "null scene" in L.rt_last_error().decode()
