"""rtnw.py — Python view of librt_hip.so (include/rt_hip.h) via ctypes.

The path tracer's product is the C ABI; this module is the host-side mirror the
tests and bench.py drive it through, named after the reference's interface:

    scene  = Scene.builtin("final")             # main.cpp:190-230 built by the host API
    cam    = Camera.preset("cornell", nx, ny)   # camera.h:21-39 (main.cpp:254-259)
    mean   = scene.render_tile(cam, RenderParams(nx=.., ny=.., spp=..), 0, 0, nx, ny)
    ppm    = ppm_text(quantize(mean))           # main.cpp:314-330

There is no CPU fallback: every render goes through the HIP megakernel, and
loading fails loudly when librt_hip.so is missing.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTNW_LIB") or os.path.join(HERE, "librt_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "rt_hip.h")

RT_OK = 0
RT_BG_BLACK, RT_BG_SKY = 0, 1
RT_FLAG_COUNT = 1
RT_FLAG_PROFILE = 2
RT_FLAG_SUM_IN = 4      # the output holds the sums of samples [0, sample_offset) on entry
RT_FLAG_SUM_OUT = 8     # write per-pixel sums (checkpoints), not means
RT_FLAG_RIGHT_FOLD = 16  # parity mode: main.cpp:36's right fold per sample (rt_hip.h)
RT_CHECKPOINT_MAGIC = 0x4B435452


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt_hip error {code}: {msg}")
        self.code = code


class RtPrim(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("material", ctypes.c_int32), ("instance", ctypes.c_int32),
                ("flip", ctypes.c_int32), ("p", ctypes.c_float * 12)]


class RtInstance(ctypes.Structure):
    _fields_ = [("nops", ctypes.c_int32), ("pad", ctypes.c_int32 * 3), ("ops", (ctypes.c_float * 4) * 6)]


class RtMaterial(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("texture", ctypes.c_int32), ("fuzz", ctypes.c_float),
                ("ref_idx", ctypes.c_float), ("albedo", ctypes.c_float * 3), ("pad", ctypes.c_int32)]


class RtTexture(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("even", ctypes.c_int32), ("odd", ctypes.c_int32),
                ("scale", ctypes.c_float), ("color", ctypes.c_float * 3), ("image", ctypes.c_int32)]


class RtMedium(ctypes.Structure):
    _fields_ = [("boundary_first", ctypes.c_int32), ("boundary_count", ctypes.c_int32), ("density", ctypes.c_float),
                ("material", ctypes.c_int32), ("order", ctypes.c_int32), ("pad", ctypes.c_int32 * 3)]


class RtImage(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32)]


class RtSceneDesc(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_uint32), ("nprims", ctypes.c_int32), ("nboundary", ctypes.c_int32),
                ("nmedia", ctypes.c_int32), ("nmaterials", ctypes.c_int32), ("ntextures", ctypes.c_int32),
                ("ninstances", ctypes.c_int32),
                ("prims", ctypes.POINTER(RtPrim)), ("boundary_prims", ctypes.POINTER(RtPrim)),
                ("media", ctypes.POINTER(RtMedium)), ("materials", ctypes.POINTER(RtMaterial)),
                ("textures", ctypes.POINTER(RtTexture)), ("instances", ctypes.POINTER(RtInstance)),
                ("perlin_ranvec", ctypes.POINTER(ctypes.c_float)), ("perlin_perm", ctypes.POINTER(ctypes.c_int32)),
                ("time0", ctypes.c_float), ("time1", ctypes.c_float),
                ("nimages", ctypes.c_int32), ("images", ctypes.POINTER(RtImage)),
                ("image_data", ctypes.POINTER(ctypes.c_uint8)), ("image_bytes", ctypes.c_int64)]


class RtCameraDesc(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_float * 3), ("lower_left_corner", ctypes.c_float * 3),
                ("horizontal", ctypes.c_float * 3), ("vertical", ctypes.c_float * 3), ("u", ctypes.c_float * 3),
                ("v", ctypes.c_float * 3), ("w", ctypes.c_float * 3), ("lens_radius", ctypes.c_float),
                ("time0", ctypes.c_float), ("time1", ctypes.c_float)]


class RtRenderParams(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("spp", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("t_min", ctypes.c_float), ("background", ctypes.c_int32), ("chunk", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("sample_offset", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("seed", ctypes.c_uint64)]


class RtStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "samples", "segments", "node_visits", "sphere_tests", "moving_sphere_tests", "rect_tests", "instanced_tests",
        "medium_tests", "shades", "noise_evals", "algorithmic_bytes", "kernel_ms", "resolve_ms",
        "cycles_claim", "cycles_traverse", "cycles_media", "cycles_shade", "grid", "wave_iterations",
        "wave_node_trips", "wave_prim_trips", "wave_sphere_draw_trips", "lane_sphere_draw_trips", "chunk",
        "batches", "lds_level", "stack_depth", "scan_groups", "prescan", "wave_exhaust_first_us",
        "wave_exhaust_last_us", "wave_end_first_us", "wave_end_mean_us", "wave_end_last_us",
        "wave_shade_passes", "wave_shade_kinds", "lane_scatters", "cycles_scatter", "ball_fused_scatters",
        "ball_fused_declined", "empty_fast_samples", "empty_pixels")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtAdaptiveParams(ctypes.Structure):
    _fields_ = [("min_spp", ctypes.c_int32), ("step_spp", ctypes.c_int32), ("tolerance", ctypes.c_float),
                ("floor", ctypes.c_float)]


class RtAdaptiveStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in (
        "passes", "samples", "pixels_converged", "pixels_capped", "kernel_ms", "resolve_ms", "select_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtDenoiseParams(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("demodulate", ctypes.c_int32), ("sigma_color", ctypes.c_float),
                ("sigma_depth", ctypes.c_float), ("uniform_spp", ctypes.c_int32), ("variance_filter", ctypes.c_int32),
                ("pad", ctypes.c_int32 * 2)]


# the denoiser's suggested settings (DESIGN.md §7c records the sweep that chose them)
DENOISE_DEFAULTS = dict(iterations=3, demodulate=1, sigma_color=2.0, sigma_depth=1.0)


class RtFireflyParams(ctypes.Structure):
    _fields_ = [("demodulate", ctypes.c_int32), ("radius", ctypes.c_int32), ("min_similar", ctypes.c_int32),
                ("k", ctypes.c_float), ("floor", ctypes.c_float), ("cos_normal", ctypes.c_float),
                ("sigma_depth", ctypes.c_float), ("sigma_albedo", ctypes.c_float)]


# the firefly clamp's suggested settings (DESIGN.md §7e records the sweep that chose them)
FIREFLY_DEFAULTS = dict(demodulate=1, radius=2, min_similar=3, k=8.0, floor=0.01, cos_normal=0.9, sigma_depth=0.1,
                        sigma_albedo=0.25)


class RtTemporalFrame(ctypes.Structure):   # the frame, the history and the output of rt_temporal
    _fields_ = [("color", ctypes.c_void_p), ("guides", ctypes.c_void_p), ("moments", ctypes.c_void_p),
                ("len", ctypes.c_void_p)]


class RtTemporalParams(ctypes.Structure):   # 32 bytes
    _fields_ = [("max_history", ctypes.c_int32), ("cos_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float),
                ("frame_spp", ctypes.c_int32), ("pad", ctypes.c_int32 * 4)]


# the frame history's suggested settings (DESIGN.md §7h records the sweep that chose max_history)
TEMPORAL_DEFAULTS = dict(max_history=16, cos_normal=0.9, sigma_depth=0.1)


class RtTemporalClampParams(ctypes.Structure):   # 32 bytes
    _fields_ = [("radius", ctypes.c_int32), ("gamma", ctypes.c_float), ("pad", ctypes.c_int32 * 6)]


# the clamped frame history's settings when none are given: no clamp.  DESIGN.md §7j records the sweep: no radius
# and gamma served random_scene without costing final() more, so radius 0 it is (radius 1, gamma 0.5 is the
# setting that gains on random_scene)
TEMPORAL_CLAMP_DEFAULTS = dict(max_history=16, radius=0, gamma=1.0)


class RtTemporalCoverParams(ctypes.Structure):   # 32 bytes
    _fields_ = [("background", ctypes.c_int32), ("edges", ctypes.c_int32), ("sigma_coverage", ctypes.c_float),
                ("pad", ctypes.c_int32 * 5)]


# where rt_temporal_cover's history came from, per pixel (rt_hip.h)
RT_TEMPORAL_SRC_NONE, RT_TEMPORAL_SRC_SURFACE, RT_TEMPORAL_SRC_BACKGROUND, RT_TEMPORAL_SRC_EDGE, RT_TEMPORAL_SRC_SAME = 0, 1, 2, 4, 8

# rt_temporal_cover's settings when none are given.  DESIGN.md §7k records the sweep: background and edges with
# sigma_coverage 0.5 lower the error on both scenes (final() 0.169 -> 0.122, random_scene 0.0345 -> 0.0340), so they
# are on; the clamp still costs final() more than it gains random_scene, so radius stays 0
TEMPORAL_COVER_DEFAULTS = dict(max_history=16, radius=0, gamma=1.0, background=1, edges=1, sigma_coverage=0.5)


class RtRay(ctypes.Structure):   # 48 bytes
    _fields_ = [("origin", ctypes.c_float * 3), ("t_min", ctypes.c_float), ("dir", ctypes.c_float * 3),
                ("t_max", ctypes.c_float), ("time", ctypes.c_float), ("pad", ctypes.c_float * 3)]


class RtHit(ctypes.Structure):   # 48 bytes
    _fields_ = [("prim", ctypes.c_int32), ("material", ctypes.c_int32), ("t", ctypes.c_float), ("depth", ctypes.c_float),
                ("normal", ctypes.c_float * 3), ("albedo", ctypes.c_float * 3), ("pad", ctypes.c_int32 * 2)]


RT_HIT_MISS, RT_HIT_INVALID = -1, -2
RT_OCCLUDED_INVALID = 255
# rt_ray and rt_hit as numpy records (the ctypes structures' layout)
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("dir", np.float32, 3), ("t_max", np.float32),
                      ("time", np.float32), ("pad", np.float32, 3)])
HIT_DTYPE = np.dtype([("prim", np.int32), ("material", np.int32), ("t", np.float32), ("depth", np.float32),
                      ("normal", np.float32, 3), ("albedo", np.float32, 3), ("pad", np.int32, 2)])


def pack_rays(origin, dir, t_min=0.001, t_max=np.inf, time=0.0) -> np.ndarray:
    """rt_ray records ([n] RAY_DTYPE) from origins and directions [n, 3] (either may be one
    vector for all) and t_min, t_max and time, scalars or [n]."""
    o = np.asarray(origin, np.float32).reshape(-1, 3)
    d = np.asarray(dir, np.float32).reshape(-1, 3)
    n = max(len(o), len(d), *(np.size(x) for x in (t_min, t_max, time)))
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"], rays["dir"] = o, d
    for name, x in (("t_min", t_min), ("t_max", t_max), ("time", time)):
        rays[name] = np.asarray(x, np.float32).reshape(-1)
    return rays


class RtPathRay(ctypes.Structure):   # 48 bytes
    _fields_ = [("origin", ctypes.c_float * 3), ("time", ctypes.c_float), ("dir", ctypes.c_float * 3),
                ("skip", ctypes.c_uint32), ("pixel", ctypes.c_uint32), ("sample", ctypes.c_uint32),
                ("pad", ctypes.c_uint32 * 2)]


class RtRadiance(ctypes.Structure):   # 16 bytes
    _fields_ = [("rgb", ctypes.c_float * 3), ("status", ctypes.c_int32)]


RT_RADIANCE_MAX_SKIP = 192
# rt_path_ray and rt_radiance as numpy records (the ctypes structures' layout)
PATH_RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("time", np.float32), ("dir", np.float32, 3), ("skip", np.uint32),
                           ("pixel", np.uint32), ("sample", np.uint32), ("pad", np.uint32, 2)])
RADIANCE_DTYPE = np.dtype([("rgb", np.float32, 3), ("status", np.int32)])


def pack_path_rays(origin, dir, time=0.0, pixel=0, sample=0, skip=0) -> np.ndarray:
    """rt_path_ray records ([n] PATH_RAY_DTYPE) from origins and directions [n, 3] (either may be
    one vector for all) and time, pixel, sample and skip, scalars or [n]: the ray, the sample
    stream's key numbers and the draws of that stream already spent (rt_hip.h)."""
    o = np.asarray(origin, np.float32).reshape(-1, 3)
    d = np.asarray(dir, np.float32).reshape(-1, 3)
    n = max(len(o), len(d), *(np.size(x) for x in (time, pixel, sample, skip)))
    rays = np.zeros(n, PATH_RAY_DTYPE)
    rays["origin"], rays["dir"] = o, d
    rays["time"] = np.asarray(time, np.float32).reshape(-1)
    for name, x in (("pixel", pixel), ("sample", sample), ("skip", skip)):
        rays[name] = np.asarray(x, np.uint32).reshape(-1)
    return rays


class RtLensParams(ctypes.Structure):   # 32 bytes
    _fields_ = [("model", ctypes.c_int32), ("fov_deg", ctypes.c_float), ("pad", ctypes.c_int32 * 6)]


RT_LENS_PERSPECTIVE, RT_LENS_ORTHOGRAPHIC, RT_LENS_FISHEYE, RT_LENS_EQUIRECT = 0, 1, 2, 3


def lens_params(model, fov_deg=180.0) -> RtLensParams:
    """rt_lens_params: a camera model (RT_LENS_*) and, for the fisheye, the full angle across
    the image circle in degrees."""
    return RtLensParams(model=int(model), fov_deg=float(fov_deg))


def _lens_count(params, w, h):
    """The records of a w x h rectangle, or ValueError: the arrays are sized before the library
    checks the arguments."""
    if w < 1 or h < 1 or params.spp < 1:
        raise ValueError("w, h and params.spp must be at least 1")
    return w * h * params.spp


def lens_rays_dev(cam, params: RtRenderParams, lens: RtLensParams, x0, y0, w, h, rays_dev_ptr: int,
                  trace_rays_dev_ptr: int = 0, stream_ptr: int = 0, device: int = 0):
    """rt_lens_rays_dev: the w x h rectangle's rt_path_ray records (and rt_ray records, when a
    pointer is given) into device memory, sample-major, enqueued on the stream."""
    _check(lib().rt_lens_rays_dev(device, ctypes.byref(cam.desc), ctypes.byref(lens), ctypes.byref(params), x0, y0, w, h,
                                  ctypes.c_void_p(rays_dev_ptr), ctypes.c_void_p(trace_rays_dev_ptr or None),
                                  ctypes.c_void_p(stream_ptr)))


def lens_rays(cam, params: RtRenderParams, lens: RtLensParams, x0, y0, w, h, trace: bool = False, device: int = 0):
    """rt_lens_rays: the camera model's rays of the w x h rectangle as [spp, h, w] PATH_RAY_DTYPE
    records (sample s of the call is params.sample_offset + s), made on the device; with trace
    also the same rays as [spp, h, w] RAY_DTYPE records (t_min = params.t_min, t_max = +inf)."""
    n = _lens_count(params, w, h)
    rays = np.zeros(n, PATH_RAY_DTYPE)
    tr = np.zeros(n, RAY_DTYPE) if trace else None
    _check(lib().rt_lens_rays(device, ctypes.byref(cam.desc), ctypes.byref(lens), ctypes.byref(params), x0, y0, w, h,
                              rays.ctypes.data, _ptr(tr)))
    shape = (params.spp, h, w)
    return (rays.reshape(shape), tr.reshape(shape)) if trace else rays.reshape(shape)


class RtCheckpoint(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("nx", ctypes.c_int32),
                ("ny", ctypes.c_int32), ("samples_done", ctypes.c_uint32), ("max_depth", ctypes.c_int32),
                ("background", ctypes.c_int32), ("t_min", ctypes.c_float), ("seed", ctypes.c_uint64),
                ("job_hash", ctypes.c_uint64), ("count", ctypes.c_uint64)]


_lib = None


def lib():
    """Loads librt_hip.so (torch first, so one HIP runtime serves both)."""
    global _lib
    if _lib is None:
        try:  # if torch is present, bind its HIP runtime (same SONAME) before ours
            import torch  # noqa: F401
        except Exception:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {HERE}` (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        sig = {
            "rt_camera_init": (ctypes.c_int, [P(RtCameraDesc), P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float),
                                              ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                              ctypes.c_float, ctypes.c_float]),
            "rt_scene_create": (ctypes.c_int, [P(RtSceneDesc), ctypes.c_int, P(ctypes.c_void_p)]),
            "rt_scene_destroy": (None, [ctypes.c_void_p]),
            "rt_render_tile": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, P(RtStats)]),
            "rt_render_tiles": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams), ctypes.c_void_p,
                                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, P(RtStats)]),
            "rt_render_tiles_moments": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams),
                                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, P(RtStats)]),
            "rt_render_adaptive": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams),
                                                  P(RtAdaptiveParams), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  P(RtAdaptiveStats)]),
            "rt_render_adaptive_guarded": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams),
                                                          P(RtAdaptiveParams), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_void_p, P(RtAdaptiveStats)]),
            "rt_copy_to_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
            "rt_render_features": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams), ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
            "rt_render_features_dev": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams), ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
            "rt_denoise": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          P(RtDenoiseParams), ctypes.c_void_p, P(ctypes.c_double)]),
            "rt_denoise_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, P(RtDenoiseParams), ctypes.c_void_p,
                                              ctypes.c_void_p]),
            "rt_firefly": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, P(RtFireflyParams),
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_double)]),
            "rt_firefly_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, P(RtFireflyParams), ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
            "rt_temporal": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(RtTemporalFrame), P(RtCameraDesc),
                                           P(RtTemporalFrame), P(RtCameraDesc), P(RtTemporalParams), P(RtTemporalFrame),
                                           P(ctypes.c_double)]),
            "rt_temporal_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(RtTemporalFrame), P(RtCameraDesc),
                                               P(RtTemporalFrame), P(RtCameraDesc), P(RtTemporalParams),
                                               P(RtTemporalFrame), ctypes.c_void_p]),
            "rt_temporal_clamped": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(RtTemporalFrame),
                                                   P(RtCameraDesc), P(RtTemporalFrame), P(RtCameraDesc), P(RtTemporalParams),
                                                   P(RtTemporalClampParams), P(RtTemporalFrame), ctypes.c_void_p,
                                                   P(ctypes.c_double)]),
            "rt_temporal_clamped_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(RtTemporalFrame),
                                                       P(RtCameraDesc), P(RtTemporalFrame), P(RtCameraDesc),
                                                       P(RtTemporalParams), P(RtTemporalClampParams), P(RtTemporalFrame),
                                                       ctypes.c_void_p, ctypes.c_void_p]),
            "rt_temporal_cover": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(RtTemporalFrame),
                                                 P(RtCameraDesc), P(RtTemporalFrame), P(RtCameraDesc), P(RtTemporalParams),
                                                 P(RtTemporalClampParams), P(RtTemporalCoverParams), P(RtTemporalFrame),
                                                 ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_double)]),
            "rt_temporal_cover_dev": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(RtTemporalFrame),
                                                     P(RtCameraDesc), P(RtTemporalFrame), P(RtCameraDesc),
                                                     P(RtTemporalParams), P(RtTemporalClampParams),
                                                     P(RtTemporalCoverParams), P(RtTemporalFrame), ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p]),
            "rt_trace_rays":(ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                             P(ctypes.c_double)]),
            "rt_trace_rays_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
            "rt_occluded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                           P(ctypes.c_double)]),
            "rt_occluded_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_void_p]),
            "rt_radiance_rays": (ctypes.c_int, [ctypes.c_void_p, P(RtRenderParams), ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, P(ctypes.c_double)]),
            "rt_radiance_rays_dev": (ctypes.c_int, [ctypes.c_void_p, P(RtRenderParams), ctypes.c_void_p, ctypes.c_int64,
                                                    ctypes.c_void_p, ctypes.c_void_p]),
            "rt_lens_rays": (ctypes.c_int, [ctypes.c_int, P(RtCameraDesc), P(RtLensParams), P(RtRenderParams), ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
            "rt_lens_rays_dev": (ctypes.c_int, [ctypes.c_int, P(RtCameraDesc), P(RtLensParams), P(RtRenderParams),
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
            "rt_render_lens": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtLensParams), P(RtRenderParams),
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_double)]),
            "rt_render_lens_dev": (ctypes.c_int, [ctypes.c_void_p, P(RtCameraDesc), P(RtLensParams), P(RtRenderParams),
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
            "rt_device_alloc": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, P(ctypes.c_void_p)]),
            "rt_device_free": (ctypes.c_int, [ctypes.c_void_p]),
            "rt_copy_to_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
            "rt_device_count": (ctypes.c_int, [P(ctypes.c_int)]),
            "rt_quantize": (None, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
            "rt_ppm_text": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]),
            "rt_builtin_scene_desc": (ctypes.c_int, [ctypes.c_char_p, P(P(RtSceneDesc))]),
            "rt_scene_desc_free": (None, [P(RtSceneDesc)]),
            "rt_scene_desc_dump": (ctypes.c_int64, [P(RtSceneDesc), ctypes.c_char_p, ctypes.c_int64]),
            "rt_checkpoint_write": (ctypes.c_int, [ctypes.c_char_p, P(RtCheckpoint), ctypes.c_void_p]),
            "rt_checkpoint_read": (ctypes.c_int, [ctypes.c_char_p, P(RtCheckpoint), ctypes.c_void_p, ctypes.c_uint64]),
            "rt_dist_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
            "rt_dist_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, P(ctypes.c_void_p)]),
            "rt_dist_destroy": (None, [ctypes.c_void_p]),
            "rt_dist_gather": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                              ctypes.c_int, ctypes.c_void_p]),
            "rt_interleave_factors": (None, [ctypes.c_int, P(ctypes.c_int), P(ctypes.c_int)]),
            "rt_rank_pixels": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_int64]),
            "rt_rank_tiles": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]),
            "rt_dist_set_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
            "rt_unpack_tiles": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p]),
            "rt_dist_render": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, P(RtCameraDesc), P(RtRenderParams),
                                              ctypes.c_void_p, P(RtStats)]),
            "rt_math_probe": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64]),
            "rt_last_error": (ctypes.c_char_p, []),
            "rt_version": (ctypes.c_char_p, []),
        }
        # what a library built before them lacks (A/B variants): diagnostics, the moments and adaptive entries,
        # the feature pass, the denoiser, the firefly clamp, the frame history, its clamped form and the one for
        # background and edge pixels, the ray queries, the radiance queries and the lens renders
        optional = {"rt_math_probe", "rt_render_tiles_moments", "rt_render_adaptive", "rt_render_adaptive_guarded",
                    "rt_copy_to_device", "rt_lens_rays", "rt_lens_rays_dev", "rt_render_lens", "rt_render_lens_dev",
                    "rt_render_features", "rt_render_features_dev", "rt_denoise", "rt_denoise_dev",
                    "rt_firefly", "rt_firefly_dev", "rt_temporal", "rt_temporal_dev",
                    "rt_temporal_clamped", "rt_temporal_clamped_dev", "rt_temporal_cover", "rt_temporal_cover_dev", "rt_trace_rays", "rt_trace_rays_dev", "rt_occluded", "rt_occluded_dev",
                    "rt_radiance_rays", "rt_radiance_rays_dev"}
        for name, (res, args) in sig.items():
            if name in optional and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


MATH_PROBE = {"sinf": 0, "sinf_ocml": 1, "asinf": 2, "asinf_ocml": 3, "atan2f": 4, "atan2f_ocml": 5}


def math_probe(fn: str, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
    """The device's float transcendentals on host inputs (rt_math_probe): `fn` one of
    MATH_PROBE (the megakernel's glibc restatements, rt_libm.h, or ocml's forms)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    bb = np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.float32)
    out = np.empty_like(a)
    _check(lib().rt_math_probe(MATH_PROBE[fn], a.ctypes.data, bb.ctypes.data, out.ctypes.data, a.size))
    return out


def _check(rc):
    if rc != RT_OK:
        raise RtError(rc, lib().rt_last_error().decode())
    return rc


def _ptr(a):
    """An optional array's address: None stays None (a null pointer)."""
    return None if a is None else a.ctypes.data


def _params(T, defaults, ints, given, **fixed):
    """The ctypes params struct T: the `given` settings, None taking its value in `defaults` and
    those named in `ints` cast with int(), beside the `fixed` fields, which have no default."""
    v = {n: defaults[n] if x is None else x for n, x in given.items()}
    return T(**{n: int(x) if n in ints else x for n, x in v.items()}, **fixed)


def _planes(features, ny, nx):
    """The albedo, normal and depth planes of a features dict (Scene.render_features')."""
    return (np.ascontiguousarray(features["albedo"], np.float32).reshape(ny, nx, 3),
            np.ascontiguousarray(features["normal"], np.float32).reshape(ny, nx, 3),
            np.ascontiguousarray(features["depth"], np.float32).reshape(ny, nx))


def header_symbols(path: str = HEADER):
    """Function names declared in include/rt_hip.h."""
    text = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(rt_\w+)\s*\(", text, flags=re.M)))


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().rt_device_count(ctypes.byref(n))
    return n.value if rc == RT_OK else 0


# --------------------------------------------------------------------- camera
CAMERA_PRESETS = {   # main.cpp:254-276
    "cornell": dict(lookfrom=(228, 278, -800), lookat=(278, 278, 0), vfov=40.0, aperture=0.0),
    "random": dict(lookfrom=(13, 2, 3), lookat=(0, 0, 0), vfov=20.0, aperture=0.1),
    "final_alt": dict(lookfrom=(478, 278, -600), lookat=(278, 278, 0), vfov=20.0, aperture=0.0),
}


class Camera:
    def __init__(self, lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, t0=0.0, t1=1.0):
        f3 = ctypes.c_float * 3
        self.desc = RtCameraDesc()
        _check(lib().rt_camera_init(ctypes.byref(self.desc), f3(*lookfrom), f3(*lookat), f3(*vup), vfov, aspect,
                                    aperture, focus_dist, t0, t1))

    @classmethod
    def preset(cls, name, nx, ny):
        p = CAMERA_PRESETS[name]
        aspect = float(np.float32(nx) / np.float32(ny))
        return cls(p["lookfrom"], p["lookat"], (0, 1, 0), p["vfov"], aspect, p["aperture"], 10.0, 0.0, 1.0)

    def as_array(self):
        d = self.desc
        return np.array(list(d.origin) + list(d.lower_left_corner) + list(d.horizontal) + list(d.vertical) +
                        list(d.u) + list(d.v) + list(d.w) + [d.lens_radius, d.time0, d.time1], dtype=np.float32)


# ---------------------------------------------------------------------- scene
SCENE_DEFAULTS = {   # per-scene camera / background / depth pairing
    "random_scene": ("random", RT_BG_SKY, 8),
    "random_motion": ("random", RT_BG_SKY, 50),
    "cornell_box": ("cornell", RT_BG_BLACK, 50),
    "cornell_smoke": ("cornell", RT_BG_BLACK, 50),
    "final": ("cornell", RT_BG_BLACK, 50),
    "simple_light": ("random", RT_BG_BLACK, 50),
    "two_spheres": ("random", RT_BG_BLACK, 50),
    "edge_empty": ("random", RT_BG_SKY, 50),        # the tests' edge scenes (oracle/ref_harness.cpp edge_*)
    "edge_single": ("random", RT_BG_SKY, 50),
    "edge_degenerate": ("random", RT_BG_SKY, 50),
    "edge_chains": ("random", RT_BG_SKY, 50),
    "test": ("random", RT_BG_BLACK, 50),
    "earth": ("cornell", RT_BG_BLACK, 50),
}


def RenderParams(nx, ny, spp, max_depth=50, t_min=0.001, background=RT_BG_BLACK, chunk=0, flags=0, seed=0,
                 sample_offset=0) -> RtRenderParams:
    return RtRenderParams(nx=nx, ny=ny, spp=spp, max_depth=max_depth, t_min=t_min, background=background,
                          chunk=chunk, flags=flags, sample_offset=sample_offset, seed=seed)


RT_ABI_VERSION = 2


class SceneDesc:
    """A flattened scene: built by the host API (owned by librt_hip), or from_arrays (owned by
    this object)."""

    def __init__(self, ptr, keep=None):
        self.ptr = ptr
        self._keep = keep   # from_arrays: the numpy arrays and the struct the pointers lead into

    @classmethod
    def from_arrays(cls, *, prims, materials, textures, perlin_ranvec, perlin_perm, boundary_prims=(), media=(),
                    instances=(), images=(), image_data=b"", time0=0.0, time1=1.0) -> "SceneDesc":
        """A descriptor over arrays this object owns.  prims, boundary_prims, media, materials,
        textures, instances and images are sequences of RtPrim, RtMedium, RtMaterial, RtTexture,
        RtInstance and RtImage; perlin_ranvec is 256 x 3 float32, perlin_perm 3 x 256 int32;
        image_data the texel bytes of all images.  The arrays live as long as the object and are
        never handed to rt_scene_desc_free."""
        def arr(items, T):
            a = (T * max(1, len(items)))()
            for i, x in enumerate(items):
                a[i] = x
            return a, len(items)
        keep = {}
        d = RtSceneDesc(abi_version=RT_ABI_VERSION, time0=time0, time1=time1)
        for field, count, items, T in (("prims", "nprims", prims, RtPrim), ("boundary_prims", "nboundary", boundary_prims, RtPrim),
                                       ("media", "nmedia", media, RtMedium), ("materials", "nmaterials", materials, RtMaterial),
                                       ("textures", "ntextures", textures, RtTexture),
                                       ("instances", "ninstances", instances, RtInstance), ("images", "nimages", images, RtImage)):
            a, n = arr(list(items), T)
            keep[field] = a
            setattr(d, field, ctypes.cast(a, ctypes.POINTER(T)))
            setattr(d, count, n)
        rv = np.ascontiguousarray(perlin_ranvec, dtype=np.float32).reshape(768)
        pm = np.ascontiguousarray(perlin_perm, dtype=np.int32).reshape(768)
        tx = np.frombuffer(bytes(image_data) or b"\0", dtype=np.uint8).copy()
        keep.update(ranvec=rv, perm=pm, texels=tx)
        d.perlin_ranvec = rv.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        d.perlin_perm = pm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        d.image_data = tx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        d.image_bytes = len(image_data)
        keep["desc"] = d
        return cls(ctypes.pointer(d), keep)

    @classmethod
    def builtin(cls, name: str, earth_png: str | None = None) -> "SceneDesc":
        """earth() reads its texture like the reference (main.cpp:93): "picture.png" in
        the working directory, or earth_png / $RTNW_EARTH_PNG."""
        if name == "earth" and earth_png:
            os.environ["RTNW_EARTH_PNG"] = earth_png
        p = ctypes.POINTER(RtSceneDesc)()
        _check(lib().rt_builtin_scene_desc(name.encode(), ctypes.byref(p)))
        return cls(p)

    def dump(self) -> str:
        n = lib().rt_scene_desc_dump(self.ptr, None, 0)
        buf = ctypes.create_string_buffer(int(n))
        lib().rt_scene_desc_dump(self.ptr, buf, n)
        return buf.raw[:n].decode()

    @property
    def contents(self) -> RtSceneDesc:
        return self.ptr.contents

    def free(self):
        if self.ptr and self._keep is None:
            lib().rt_scene_desc_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Scene:
    """A scene resident in one GPU's HBM (rt_scene_create)."""

    def __init__(self, desc: SceneDesc, device: int = 0):
        self.desc = desc
        self.handle = ctypes.c_void_p()
        _check(lib().rt_scene_create(desc.ptr, device, ctypes.byref(self.handle)))

    @classmethod
    def builtin(cls, name: str, device: int = 0, earth_png: str | None = None) -> "Scene":
        return cls(SceneDesc.builtin(name, earth_png), device)

    def render_tile(self, cam: Camera, params: RtRenderParams, x0, y0, w, h, stats: bool = False, sums=None):
        """Mean radiance of the w x h tile ([h, w, 3] float32).  With RT_FLAG_SUM_IN,
        `sums` holds the running sums of samples [0, params.sample_offset) (e.g. from
        read_checkpoint); with RT_FLAG_SUM_OUT the result is sums, not means."""
        out = np.zeros((h, w, 3), dtype=np.float32)
        if params.flags & RT_FLAG_SUM_IN:
            if sums is None:
                raise ValueError("RT_FLAG_SUM_IN needs the running sums")
            out[...] = np.asarray(sums, np.float32).reshape(h, w, 3)
        st = RtStats()
        _check(lib().rt_render_tile(self.handle, ctypes.byref(cam.desc), ctypes.byref(params), x0, y0, w, h,
                                    out.ctypes.data, ctypes.byref(st)))
        return (out, st.as_dict()) if stats else out

    def render_tiles(self, cam: Camera, params: RtRenderParams, tiles, out_dev_ptr: int, stream_ptr: int = 0,
                     stats: bool = True):
        t = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4))
        st = RtStats()
        _check(lib().rt_render_tiles(self.handle, ctypes.byref(cam.desc), ctypes.byref(params), t.ctypes.data,
                                     int(t.shape[0]), ctypes.c_void_p(out_dev_ptr), ctypes.c_void_p(stream_ptr),
                                     ctypes.byref(st) if stats else None))
        return st.as_dict()

    def render_tile_moments(self, cam: Camera, params: RtRenderParams, x0, y0, w, h, stats: bool = False, sums=None,
                            moments=None, device: int = 0):
        """render_tile plus the tile's moments ([h, w, 2] float32: per pixel the sum and the sum
        of squares of the work items' y = (r + g) + b; rt_render_tiles_moments).  With
        RT_FLAG_SUM_IN, `sums` and `moments` hold the earlier samples' values."""
        L = lib()
        out = np.zeros((h, w, 3), dtype=np.float32)
        mom = np.zeros((h, w, 2), dtype=np.float32)
        sum_in = bool(params.flags & RT_FLAG_SUM_IN)
        if sum_in:
            if sums is None or moments is None:
                raise ValueError("RT_FLAG_SUM_IN needs the running sums and moments")
            out[...] = np.asarray(sums, np.float32).reshape(h, w, 3)
            mom[...] = np.asarray(moments, np.float32).reshape(h, w, 2)
        dev = ctypes.c_void_p()
        _check(L.rt_device_alloc(device, out.nbytes + mom.nbytes, ctypes.byref(dev)))
        try:
            dmom = ctypes.c_void_p(dev.value + out.nbytes)
            if sum_in:
                _check(L.rt_copy_to_device(dev, out.ctypes.data, out.nbytes))
                _check(L.rt_copy_to_device(dmom, mom.ctypes.data, mom.nbytes))
            tile = (ctypes.c_int32 * 4)(x0, y0, w, h)
            st = RtStats()
            _check(L.rt_render_tiles_moments(self.handle, ctypes.byref(cam.desc), ctypes.byref(params), tile, 1, dev, dmom,
                                             None, ctypes.byref(st)))
            _check(L.rt_copy_to_host(out.ctypes.data, dev, out.nbytes))
            _check(L.rt_copy_to_host(mom.ctypes.data, dmom, mom.nbytes))
        finally:
            L.rt_device_free(dev)
        return (out, mom, st.as_dict()) if stats else (out, mom)

    def render_adaptive(self, cam: Camera, params: RtRenderParams, x0, y0, w, h, *, min_spp, step_spp, tolerance,
                        floor=0.0, guard_radius=None):
        """Error-driven render (rt_render_adaptive; params.spp is the cap): returns the mean
        [h, w, 3], each pixel's sample count [h, w] int32, its moments [h, w, 2] and the
        rt_adaptive_stats as a dict.  guard_radius: None, or 0..8 for
        rt_render_adaptive_guarded: a pixel stops only when no pixel within that many pixels
        of it, inside the rectangle, fails its own test."""
        ap = RtAdaptiveParams(min_spp=min_spp, step_spp=step_spp, tolerance=tolerance, floor=floor)
        out = np.zeros((h, w, 3), dtype=np.float32)
        spp = np.zeros((h, w), dtype=np.int32)
        mom = np.zeros((h, w, 2), dtype=np.float32)
        st = RtAdaptiveStats()
        if guard_radius is None:
            _check(lib().rt_render_adaptive(self.handle, ctypes.byref(cam.desc), ctypes.byref(params), ctypes.byref(ap),
                                            x0, y0, w, h, out.ctypes.data, spp.ctypes.data, mom.ctypes.data,
                                            ctypes.byref(st)))
        else:
            _check(lib().rt_render_adaptive_guarded(self.handle, ctypes.byref(cam.desc), ctypes.byref(params),
                                                    ctypes.byref(ap), int(guard_radius), x0, y0, w, h, out.ctypes.data,
                                                    spp.ctypes.data, mom.ctypes.data, ctypes.byref(st)))
        return out, spp, mom, st.as_dict()

    def render_features(self, cam: Camera, params: RtRenderParams, x0, y0, w, h):
        """First-hit feature buffers of the w x h rectangle (rt_render_features): a dict of the
        per-pixel means over params.spp samples of `albedo` [h, w, 3], `normal` [h, w, 3],
        `depth` [h, w] and `coverage` [h, w], float32.  Constant media are seen through."""
        f = dict(albedo=np.zeros((h, w, 3), np.float32), normal=np.zeros((h, w, 3), np.float32),
                 depth=np.zeros((h, w), np.float32), coverage=np.zeros((h, w), np.float32))
        _check(lib().rt_render_features(self.handle, ctypes.byref(cam.desc), ctypes.byref(params), x0, y0, w, h,
                                        f["albedo"].ctypes.data, f["normal"].ctypes.data, f["depth"].ctypes.data,
                                        f["coverage"].ctypes.data))
        return f

    def render_features_dev(self, cam: Camera, params: RtRenderParams, x0, y0, w, h, guides_dev_ptr: int,
                            stream_ptr: int = 0):
        """rt_render_features_dev: the packed guides (8 floats per pixel: albedo.rgb, coverage,
        normal.xyz, depth) into device memory, enqueued on the stream."""
        _check(lib().rt_render_features_dev(self.handle, ctypes.byref(cam.desc), ctypes.byref(params), x0, y0, w, h,
                                            ctypes.c_void_p(guides_dev_ptr), ctypes.c_void_p(stream_ptr)))

    @staticmethod
    def _rays(rays) -> np.ndarray:
        r = np.ascontiguousarray(rays)
        if r.dtype != RAY_DTYPE:
            raise TypeError("rays must be rt_ray records (RAY_DTYPE; see pack_rays)")
        return r.reshape(-1)

    def trace_rays(self, rays, timing: bool = False):
        """Closest hit of each rt_ray record (pack_rays) by rt_trace_rays: a dict of numpy
        arrays, `prim` and `material` [n] int32 (prim -1: miss, -2: invalid ray), `t` and
        `depth` [n], `normal` and `albedo` [n, 3] float32, and `pad` [n, 2] int32 (zeros).
        timing: also the kernels' HIP-event time in ms."""
        r = self._rays(rays)
        hits = np.zeros(len(r), HIT_DTYPE)
        ms = ctypes.c_double(0.0)
        _check(lib().rt_trace_rays(self.handle, r.ctypes.data, len(r), hits.ctypes.data, ctypes.byref(ms)))
        out = {k: np.ascontiguousarray(hits[k]) for k in HIT_DTYPE.names}
        return (out, ms.value) if timing else out

    def occluded(self, rays, timing: bool = False):
        """rt_occluded: [n] uint8, 1 where the ray hits a surface between its t_min and t_max,
        0 where not, 255 for an invalid ray."""
        r = self._rays(rays)
        out = np.zeros(len(r), np.uint8)
        ms = ctypes.c_double(0.0)
        _check(lib().rt_occluded(self.handle, r.ctypes.data, len(r), out.ctypes.data, ctypes.byref(ms)))
        return (out, ms.value) if timing else out

    def trace_rays_dev(self, rays_dev_ptr: int, n: int, hits_dev_ptr: int, stream_ptr: int = 0):
        """rt_trace_rays_dev: n rt_ray records in device memory into n rt_hit records there."""
        _check(lib().rt_trace_rays_dev(self.handle, ctypes.c_void_p(rays_dev_ptr), n, ctypes.c_void_p(hits_dev_ptr),
                                       ctypes.c_void_p(stream_ptr)))

    def occluded_dev(self, rays_dev_ptr: int, n: int, out_dev_ptr: int, stream_ptr: int = 0):
        """rt_occluded_dev: n rt_ray records in device memory into n bytes there."""
        _check(lib().rt_occluded_dev(self.handle, ctypes.c_void_p(rays_dev_ptr), n, ctypes.c_void_p(out_dev_ptr),
                                     ctypes.c_void_p(stream_ptr)))

    def radiance_rays(self, params: RtRenderParams, rays, timing: bool = False):
        """rt_radiance_rays: the path-traced radiance of each rt_path_ray record (pack_path_rays)
        as [n] RADIANCE_DTYPE records (`rgb` [n, 3] float32, `status` 0 or RT_HIT_INVALID).  From
        params: max_depth, t_min, background, seed.  timing: also the kernels' HIP-event ms."""
        r = np.ascontiguousarray(rays)
        if r.dtype != PATH_RAY_DTYPE:
            raise TypeError("rays must be rt_path_ray records (PATH_RAY_DTYPE; see pack_path_rays)")
        r = r.reshape(-1)
        out = np.zeros(len(r), RADIANCE_DTYPE)
        ms = ctypes.c_double(0.0)
        _check(lib().rt_radiance_rays(self.handle, ctypes.byref(params), r.ctypes.data, len(r), out.ctypes.data,
                                      ctypes.byref(ms)))
        return (out, ms.value) if timing else out

    def radiance_rays_dev(self, params: RtRenderParams, rays_dev_ptr: int, n: int, out_dev_ptr: int, stream_ptr: int = 0):
        """rt_radiance_rays_dev: n rt_path_ray records in device memory into n rt_radiance records there."""
        _check(lib().rt_radiance_rays_dev(self.handle, ctypes.byref(params), ctypes.c_void_p(rays_dev_ptr), n,
                                          ctypes.c_void_p(out_dev_ptr), ctypes.c_void_p(stream_ptr)))

    def render_lens(self, cam: Camera, params: RtRenderParams, lens: RtLensParams, x0, y0, w, h, moments: bool = False,
                    guides: bool = False, timing: bool = False):
        """rt_render_lens: the w x h rectangle through the camera model `lens` (lens_params): the
        mean radiance [h, w, 3] float32, then — a tuple when more than the image — the moments
        [h, w, 2] with moments=True, the packed guides [h, w, 8] (pack_guides' layout) with
        guides=True and the batches' HIP-event ms with timing=True."""
        _lens_count(params, w, h)
        out = np.zeros((h, w, 3), np.float32)
        mom = np.zeros((h, w, 2), np.float32) if moments else None
        gd = np.zeros((h, w, 8), np.float32) if guides else None
        ms = ctypes.c_double(0.0)
        _check(lib().rt_render_lens(self.handle, ctypes.byref(cam.desc), ctypes.byref(lens), ctypes.byref(params), x0, y0, w, h,
                                    out.ctypes.data, _ptr(mom), _ptr(gd), ctypes.byref(ms)))
        res = [out] + ([mom] if moments else []) + ([gd] if guides else []) + ([ms.value] if timing else [])
        return res[0] if len(res) == 1 else tuple(res)

    def render_lens_dev(self, cam: Camera, params: RtRenderParams, lens: RtLensParams, x0, y0, w, h, out_dev_ptr: int,
                        moments_dev_ptr: int = 0, guides_dev_ptr: int = 0, stream_ptr: int = 0):
        """rt_render_lens_dev: the same into device memory (3, 2 and 8 floats per pixel; a zero
        pointer: not wanted), enqueued on the stream."""
        _check(lib().rt_render_lens_dev(self.handle, ctypes.byref(cam.desc), ctypes.byref(lens), ctypes.byref(params), x0, y0,
                                        w, h, ctypes.c_void_p(out_dev_ptr), ctypes.c_void_p(moments_dev_ptr or None),
                                        ctypes.c_void_p(guides_dev_ptr or None), ctypes.c_void_p(stream_ptr)))

    def close(self):
        if self.handle:
            lib().rt_scene_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------- denoiser
def denoise_params(iterations=None, demodulate=None, sigma_color=None, sigma_depth=None, uniform_spp=0,
                   variance_filter=0):
    given = dict(iterations=iterations, demodulate=demodulate, sigma_color=sigma_color, sigma_depth=sigma_depth)
    return _params(RtDenoiseParams, DENOISE_DEFAULTS, ("demodulate",), given, uniform_spp=uniform_spp,
                   variance_filter=int(variance_filter))


def denoise(color, features, moments=None, spp=None, *, iterations=None, demodulate=None, sigma_color=None,
            sigma_depth=None, variance_filter=0, device: int = 0, timing: bool = False):
    """Variance-guided edge-avoiding à-trous filter (rt_denoise) of `color` [ny, nx, 3]:
    `features` is Scene.render_features' dict (albedo, normal, depth); `moments` [ny, nx, 2]
    (render_tile_moments / render_adaptive) turns the luminance weight on, with `spp` either
    a per-pixel int32 map [ny, nx] or one count for every pixel; variance_filter=1 measures
    that weight against the 3 x 3 Gaussian of the variance instead of the centre's own.
    Unset settings take DENOISE_DEFAULTS.  Returns the filtered image (and the kernels' ms with timing=True)."""
    c = np.ascontiguousarray(color, np.float32)
    ny, nx, _ = c.shape
    a, n, z = _planes(features, ny, nx)
    m = None if moments is None else np.ascontiguousarray(moments, np.float32).reshape(ny, nx, 2)
    smap, uniform = None, 0
    if spp is not None and np.ndim(spp) == 0:
        uniform = int(spp)
    elif spp is not None:
        smap = np.ascontiguousarray(spp, np.int32).reshape(ny, nx)
    dp = denoise_params(iterations, demodulate, sigma_color, sigma_depth, uniform, variance_filter)
    out = np.zeros_like(c)
    ms = ctypes.c_double(0.0)
    _check(lib().rt_denoise(device, nx, ny, c.ctypes.data, a.ctypes.data, n.ctypes.data, z.ctypes.data,
                            _ptr(m), _ptr(smap), ctypes.byref(dp), out.ctypes.data, ctypes.byref(ms)))
    return (out, ms.value) if timing else out


# -------------------------------------------------------------- firefly clamp
def firefly_params(demodulate=None, radius=None, min_similar=None, k=None, floor=None, cos_normal=None,
                   sigma_depth=None, sigma_albedo=None):
    given = dict(demodulate=demodulate, radius=radius, min_similar=min_similar, k=k, floor=floor,
                 cos_normal=cos_normal, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo)
    return _params(RtFireflyParams, FIREFLY_DEFAULTS, ("demodulate", "radius", "min_similar"), given)


def firefly(color, features, moments=None, *, demodulate=None, radius=None, min_similar=None, k=None, floor=None,
            cos_normal=None, sigma_depth=None, sigma_albedo=None, device: int = 0, timing: bool = False,
            want_ratio: bool = False):
    """Guide-aware firefly clamp (rt_firefly) of `color` [ny, nx, 3], to run ahead of `denoise`:
    a pixel whose demodulated luminance exceeds k times the mean of its similar neighbours
    (normal, depth and albedo of `features`, Scene.render_features' dict, within `radius`)
    plus `floor` is scaled down to that bound, when it has at least `min_similar` of them.
    `moments` [ny, nx, 2] are scaled along, so they feed `denoise` unchanged.  Unset settings
    take FIREFLY_DEFAULTS.  Returns the clamped image, then the moments when `moments` was
    given, the per-pixel scale [ny, nx] with want_ratio=True and the kernel's ms with
    timing=True (a tuple when more than the image)."""
    c = np.ascontiguousarray(color, np.float32)
    ny, nx, _ = c.shape
    a, n, z = _planes(features, ny, nx)
    m = None if moments is None else np.ascontiguousarray(moments, np.float32).reshape(ny, nx, 2)
    fp = firefly_params(demodulate, radius, min_similar, k, floor, cos_normal, sigma_depth, sigma_albedo)
    out = np.zeros_like(c)
    om = None if m is None else np.zeros_like(m)
    ratio = np.zeros((ny, nx), np.float32) if want_ratio else None
    ms = ctypes.c_double(0.0)
    _check(lib().rt_firefly(device, nx, ny, c.ctypes.data, a.ctypes.data, n.ctypes.data, z.ctypes.data,
                            _ptr(m), ctypes.byref(fp), out.ctypes.data, _ptr(om), _ptr(ratio), ctypes.byref(ms)))
    res = [out] + ([om] if om is not None else []) + ([ratio] if want_ratio else []) + ([ms.value] if timing else [])
    return res[0] if len(res) == 1 else tuple(res)


# -------------------------------------------------------------- frame history
def temporal_params(frame_spp, max_history=None, cos_normal=None, sigma_depth=None):
    given = dict(max_history=max_history, cos_normal=cos_normal, sigma_depth=sigma_depth)
    return _params(RtTemporalParams, TEMPORAL_DEFAULTS, ("max_history",), given, frame_spp=int(frame_spp))


def pack_guides(features) -> np.ndarray:
    """The packed guides [ny, nx, 8] float32 (albedo.rgb, coverage, normal.xyz, depth:
    rt_render_features_dev's layout) of Scene.render_features' dict; an array of that shape
    passes through."""
    if not isinstance(features, dict):
        g = np.ascontiguousarray(features, np.float32)
        if g.ndim != 3 or g.shape[-1] != 8:
            raise ValueError("packed guides are [ny, nx, 8]")
        return g
    z = np.asarray(features["depth"], np.float32)
    g = np.zeros(z.shape + (8,), np.float32)
    g[..., 0:3] = np.asarray(features["albedo"], np.float32).reshape(z.shape + (3,))
    g[..., 3] = np.asarray(features["coverage"], np.float32).reshape(z.shape)
    g[..., 4:7] = np.asarray(features["normal"], np.float32).reshape(z.shape + (3,))
    g[..., 7] = z
    return g


def temporal_clamp_params(radius=None, gamma=None):
    return _params(RtTemporalClampParams, TEMPORAL_CLAMP_DEFAULTS, ("radius",), dict(radius=radius, gamma=gamma))


def temporal_cover_params(background=None, edges=None, sigma_coverage=None):
    given = dict(background=background, edges=edges, sigma_coverage=sigma_coverage)
    return _params(RtTemporalCoverParams, TEMPORAL_COVER_DEFAULTS, ("background", "edges"), given)


def _temporal(color, features, moments, cam, history, prev_cam, tp, cp, device, vp=None):
    """rt_temporal (cp None), rt_temporal_clamped or (with vp) rt_temporal_cover on host arrays:
    (color, moments or None, len, clipped or None, the kernel's ms), and source after them with vp."""
    c = np.ascontiguousarray(color, np.float32)
    ny, nx, _ = c.shape
    g = pack_guides(features).reshape(ny, nx, 8)
    m = None if moments is None else np.ascontiguousarray(moments, np.float32).reshape(ny, nx, 2)
    out, om, ol = np.zeros_like(c), (None if m is None else np.zeros_like(m)), np.zeros((ny, nx), np.int32)
    cur = RtTemporalFrame(_ptr(c), _ptr(g), _ptr(m), None)
    dst = RtTemporalFrame(_ptr(out), None, _ptr(om), _ptr(ol))
    hist, keep = None, None
    if history is not None:
        if prev_cam is None:
            raise ValueError("a history needs the camera it was rendered through (prev_cam)")
        hm = history.get("moments")
        keep = (np.ascontiguousarray(history["color"], np.float32).reshape(ny, nx, 3),
                pack_guides(history["features"]).reshape(ny, nx, 8),
                None if hm is None else np.ascontiguousarray(hm, np.float32).reshape(ny, nx, 2),
                np.ascontiguousarray(history["len"], np.int32).reshape(ny, nx))
        hist = RtTemporalFrame(*(_ptr(a) for a in keep))
    ms = ctypes.c_double(0.0)
    head = (device, nx, ny, ctypes.byref(cur), ctypes.byref(cam.desc), None if hist is None else ctypes.byref(hist),
            None if prev_cam is None else ctypes.byref(prev_cam.desc), ctypes.byref(tp))
    clipped = None
    if cp is None:
        _check(lib().rt_temporal(*head, ctypes.byref(dst), ctypes.byref(ms)))
    elif vp is not None:
        clipped, source = np.zeros((ny, nx), np.int32), np.zeros((ny, nx), np.int32)
        _check(lib().rt_temporal_cover(*head, ctypes.byref(cp), ctypes.byref(vp), ctypes.byref(dst), clipped.ctypes.data,
                                       source.ctypes.data, ctypes.byref(ms)))
        return out, om, ol, clipped, ms.value, source
    else:
        clipped = np.zeros((ny, nx), np.int32)
        _check(lib().rt_temporal_clamped(*head, ctypes.byref(cp), ctypes.byref(dst), clipped.ctypes.data, ctypes.byref(ms)))
    return out, om, ol, clipped, ms.value


def temporal(color, features, moments, frame_spp, cam: Camera, history=None, prev_cam: Camera | None = None, *,
             max_history=None, cos_normal=None, sigma_depth=None, device: int = 0, timing: bool = False):
    """Temporal accumulation (rt_temporal) of the frame `color` [ny, nx, 3] of `frame_spp`
    samples per pixel, rendered through `cam`, to run ahead of `denoise`: `features` is
    Scene.render_features' dict (with its coverage) or the packed guides, `moments` [ny, nx, 2]
    or None.  `history` is None for a first frame, else a dict of the previous call's results
    and that frame's features: color, moments (None when this call has none), len and features,
    seen through `prev_cam`.  Every frame must draw fresh samples (sample_offset advanced by
    frame_spp).  Unset settings take TEMPORAL_DEFAULTS.  Returns (color, moments or None, len):
    len [ny, nx] int32 is what `denoise` takes as its spp map (and the kernel's ms after them
    with timing=True)."""
    tp = temporal_params(frame_spp, max_history, cos_normal, sigma_depth)
    out, om, ol, _, ms = _temporal(color, features, moments, cam, history, prev_cam, tp, None, device)
    return (out, om, ol, ms) if timing else (out, om, ol)


def temporal_clamped(color, features, moments, frame_spp, cam: Camera, history=None, prev_cam: Camera | None = None, *,
                     radius=None, gamma=None, max_history=None, cos_normal=None, sigma_depth=None, device: int = 0,
                     timing: bool = False):
    """`temporal` with the reprojected history colour clipped to the colour box of the frame's
    neighbourhood (rt_temporal_clamped): the window's mean +- `gamma` standard deviations per
    channel, over the pixels within `radius` (0..3; 0 is `temporal` itself).  Unset radius, gamma
    and max_history take TEMPORAL_CLAMP_DEFAULTS, the others TEMPORAL_DEFAULTS.  Returns (color,
    moments or None, len, clipped): clipped [ny, nx] int32 has bit c set where channel c of the
    pixel's history colour was moved (and the kernel's ms after them with timing=True)."""
    tp = temporal_params(frame_spp, TEMPORAL_CLAMP_DEFAULTS["max_history"] if max_history is None else max_history,
                         cos_normal, sigma_depth)
    res = _temporal(color, features, moments, cam, history, prev_cam, tp, temporal_clamp_params(radius, gamma), device)
    return res if timing else res[:4]


def temporal_cover(color, features, moments, frame_spp, cam: Camera, history=None, prev_cam: Camera | None = None, *,
                   background=None, edges=None, sigma_coverage=None, radius=None, gamma=None, max_history=None,
                   cos_normal=None, sigma_depth=None, device: int = 0, timing: bool = False):
    """`temporal_clamped` with a history for the pixels it gives none under a moving camera
    (rt_temporal_cover): with `background` 1 a pixel that misses the geometry takes its history
    by direction, with `edges` 1 a partly covered pixel takes the class of its dominant part
    (surface from coverage 0.5 on), and a tap counts only when its coverage is within
    `sigma_coverage` of the pixel's.  Unset settings take TEMPORAL_COVER_DEFAULTS, cos_normal and
    sigma_depth TEMPORAL_DEFAULTS.  Returns (color, moments or None, len, clipped, source): source
    [ny, nx] int32 says where a pixel's history came from (RT_TEMPORAL_SRC_*: 0 none, 1 surface,
    2 background, 4 or'ed in on a partly covered pixel, 8 its own pixel under equal cameras) (and
    the kernel's ms after them with timing=True)."""
    d = TEMPORAL_COVER_DEFAULTS
    tp = temporal_params(frame_spp, d["max_history"] if max_history is None else max_history, cos_normal, sigma_depth)
    cp = temporal_clamp_params(d["radius"] if radius is None else radius, d["gamma"] if gamma is None else gamma)
    out, om, ol, clipped, ms, source = _temporal(color, features, moments, cam, history, prev_cam, tp, cp, device,
                                                 temporal_cover_params(background, edges, sigma_coverage))
    return (out, om, ol, clipped, source, ms) if timing else (out, om, ol, clipped, source)


# ------------------------------------------------------------ multi-GPU (RCCL)
RT_DIST_ID_BYTES = 128


def dist_unique_id() -> bytes:
    """ncclGetUniqueId (rt_dist_unique_id): created on the root, handed to every rank."""
    buf = ctypes.create_string_buffer(RT_DIST_ID_BYTES)
    _check(lib().rt_dist_unique_id(buf))
    return buf.raw


class Dist:
    """One rank's RCCL communicator (rt_dist_init = ncclCommInitRank)."""

    def __init__(self, uid: bytes, rank: int, world: int, device: int):
        assert len(uid) == RT_DIST_ID_BYTES
        self.rank, self.world = rank, world
        self.handle = ctypes.c_void_p()
        _check(lib().rt_dist_init(ctypes.create_string_buffer(uid, RT_DIST_ID_BYTES), rank, world, device,
                                  ctypes.byref(self.handle)))

    def gather(self, send_dev: int, count: int, recv_dev: int, root: int = 0, stream: int = 0):
        """ncclGather (rccl.h:745) of `count` floats per rank to `root` (world x count floats)."""
        _check(lib().rt_dist_gather(self.handle, ctypes.c_void_p(send_dev), count, ctypes.c_void_p(recv_dev), root,
                                    ctypes.c_void_p(stream)))

    def set_layout(self, layout: int):
        """rt_dist_set_layout: the split rt_dist_render uses (RT_LAYOUT_*; blocks by default)."""
        _check(lib().rt_dist_set_layout(self.handle, layout))

    def render(self, scene: "Scene", cam: "Camera", params: RtRenderParams):
        """rt_dist_render: this rank's pixels -> render -> gather; the image on rank 0."""
        img = np.zeros((params.ny, params.nx, 3), np.float32) if self.rank == 0 else None
        st = RtStats()
        _check(lib().rt_dist_render(self.handle, scene.handle, ctypes.byref(cam.desc), ctypes.byref(params),
                                    _ptr(img), ctypes.byref(st)))
        return img, st.as_dict()

    def close(self):
        if self.handle:
            lib().rt_dist_destroy(self.handle)
            self.handle = ctypes.c_void_p()


def rank_pixels_c(nx, ny, rank, world):
    """The C ABI's pixel interleave (rt_rank_pixels); equals pixels_for_rank."""
    n = lib().rt_rank_pixels(nx, ny, rank, world, None, 0)
    _check(0 if n >= 0 else int(n))
    t = np.zeros((n, 4), np.int32)
    _check(0 if lib().rt_rank_pixels(nx, ny, rank, world, t.ctypes.data, n) == n else -1)
    return t


# include/rt_hip.h RT_LAYOUT_*: how a job's pixels are split over the ranks
RT_LAYOUT_BLOCKS, RT_LAYOUT_INTERLEAVED, RT_LAYOUT_LATTICE = 0, 1, 2
RT_LAYOUT_BLOCK = 8


def rank_tiles_c(nx, ny, rank, world, layout, block=RT_LAYOUT_BLOCK):
    """The C ABI's rank share (rt_rank_tiles) as 1x1 tiles in claim order."""
    n = lib().rt_rank_tiles(nx, ny, rank, world, layout, block, None, 0)
    _check(0 if n >= 0 else int(n))
    t = np.zeros((n, 4), np.int32)
    _check(0 if lib().rt_rank_tiles(nx, ny, rank, world, layout, block, t.ctypes.data, n) == n else -1)
    return t


# ------------------------------------------------------- checkpoint / resume
def write_checkpoint(path: str, sums: np.ndarray, *, nx, ny, samples_done, params: RtRenderParams | None = None,
                     job_hash: int = 0):
    """Persists per-pixel sums (rt_checkpoint_write: atomic replace, checksummed)."""
    a = np.ascontiguousarray(sums, dtype=np.float32)
    h = RtCheckpoint(nx=nx, ny=ny, samples_done=samples_done, job_hash=job_hash, count=a.size)
    if params is not None:
        h.max_depth, h.background, h.t_min, h.seed = params.max_depth, params.background, params.t_min, params.seed
    _check(lib().rt_checkpoint_write(os.fsencode(path), ctypes.byref(h), a.ctypes.data))


def read_checkpoint(path: str):
    """Returns (header dict, float32 sums) of a checkpoint file."""
    h = RtCheckpoint()
    _check(lib().rt_checkpoint_read(os.fsencode(path), ctypes.byref(h), None, 0))
    a = np.zeros(h.count, np.float32)
    _check(lib().rt_checkpoint_read(os.fsencode(path), ctypes.byref(h), a.ctypes.data, a.size))
    return {n: getattr(h, n) for n, _ in h._fields_}, a


# -------------------------------------------------------------------- resolve
def quantize(mean: np.ndarray) -> np.ndarray:
    m = np.ascontiguousarray(mean, dtype=np.float32)
    out = np.zeros(m.shape, dtype=np.uint8)
    lib().rt_quantize(m.ctypes.data, m.size // 3, out.ctypes.data)
    return out


def ppm_text(rgb: np.ndarray) -> bytes:
    r = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = r.shape
    n = lib().rt_ppm_text(r.ctypes.data, w, h, None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib().rt_ppm_text(r.ctypes.data, w, h, buf, n)
    return buf.raw[:n]


def _mix64(z):
    M = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def tiles_for_rank(nx, ny, tile, rank, world, order="diagonal"):
    """Tiles of one rank, in raster order.
    order="diagonal": tile (tx, ty) goes to rank (tx + ty) % world.  Neighbouring
      tiles land on different ranks and the narrow edge tiles rotate over the ranks.
    order="hashed": the tiles are ranked by a hash of their raster index and dealt
      round-robin, so every rank holds the same number of tiles (+-1) scattered
      uniformly over the image: its expected path cost is the image mean whatever
      the scene's spatial structure (bench.py uses 8x8 tiles = one wave claim)."""
    cols = (nx + tile - 1) // tile
    rows = (ny + tile - 1) // tile
    if order == "hashed":
        ranked = sorted(range(cols * rows), key=lambda i: (_mix64(i ^ 0x243F6A8885A308D3), i))
        mine = sorted(ranked[rank::world])
    elif order == "diagonal":
        mine = [ty * cols + tx for ty in range(rows) for tx in range(cols) if (tx + ty) % world == rank]
    else:
        raise ValueError(f"unknown tile order {order!r}")
    out = []
    for i in mine:
        x0, y0 = (i % cols) * tile, (i // cols) * tile
        out.append((x0, y0, min(tile, nx - x0), min(tile, ny - y0)))
    return out


def interleave_factors(world):
    """world = a x b with a >= b as close to square as possible (8 -> 4 x 2)."""
    b = int(world ** 0.5)
    while world % b:
        b -= 1
    return world // b, b


def pixels_for_rank(nx, ny, rank, world, block=8):
    """Pixel interleave: with world = a x b, rank (ry, rx) = divmod(rank, a) renders
    the pixels x = rx (mod a), y = ry (mod b) — a sub-sampled copy of the whole view,
    so every rank's expected path cost is the image mean, whatever the scene's
    spatial structure.  Returned as 1x1 tiles in the order of the rank's
    sub-lattice: bands of `block` rows, each listed column by column, so ANY
    64 consecutive pixels (one wave claim, wherever it starts) cover 8 neighbouring
    columns of one band (two bands at a band's end)."""
    a, b = interleave_factors(world)
    ry, rx = divmod(rank, a)
    xs = np.arange(rx, nx, a, dtype=np.int64)
    ys = np.arange(ry, ny, b, dtype=np.int64)
    if xs.size == 0 or ys.size == 0:
        return np.zeros((0, 4), np.int32)
    J, I = np.meshgrid(np.arange(ys.size), np.arange(xs.size), indexing="ij")
    key = ((J // block) * xs.size + I) * block + J % block
    o = np.argsort(key.ravel(), kind="stable")
    t = np.ones((o.size, 4), np.int32)
    t[:, 0] = xs[I.ravel()[o]]
    t[:, 1] = ys[J.ravel()[o]]
    return t


def blocks_for_rank(nx, ny, rank, world, block=RT_LAYOUT_BLOCK):
    """Block deal (the C ABI's rt_rank_tiles, RT_LAYOUT_BLOCKS — what rt_dist_render and
    bench.py split a job by): the image's block x block pixel blocks, in Hilbert-curve
    order, dealt to the ranks in turn (block k to rank k mod world) — every rank's blocks
    spread evenly over the view (equal counts +-1), and each block keeps the 1-GPU
    render's ray coherence: a wave's 64 items are one 8 x 8 block (pixels_for_rank's
    lattice spreads them over a x 8 by b x 8 pixels).  Returned as 1x1 tiles, block by
    block, each block column by column."""
    return rank_tiles_c(nx, ny, rank, world, RT_LAYOUT_BLOCKS, block)


def lattice_blocks_for_rank(nx, ny, rank, world, block=RT_LAYOUT_BLOCK):
    """Block lattice (rt_rank_tiles, RT_LAYOUT_LATTICE): with world = a x b, rank
    (ry, rx) = divmod(rank, a) renders the block x block pixel blocks (bx, by) with
    bx = rx (mod a), by = ry (mod b) — the pixel interleave's regular sub-sampling of the
    view at block granularity, so each wave's 64 items stay one 8 x 8 block.  Returned as
    1x1 tiles, block by block in row-major block order, each block column by column."""
    return rank_tiles_c(nx, ny, rank, world, RT_LAYOUT_LATTICE, block)


def rank_layout(nx, ny, tile, world, order="diagonal"):
    """Tiles and packed float counts of every rank."""
    if order in ("interleaved", "blocks", "lattice"):   # 1x1 tiles (blocks, lattice: rt_rank_tiles)
        fn = {"blocks": blocks_for_rank, "lattice": lattice_blocks_for_rank}.get(order, pixels_for_rank)
        tiles = [fn(nx, ny, r, world) for r in range(world)]
        return tiles, [len(t) * 3 for t in tiles]
    tiles = [tiles_for_rank(nx, ny, tile, r, world, order) for r in range(world)]
    counts = [sum(w * h for _, _, w, h in t) * 3 for t in tiles]
    return tiles, counts


def unpack_tiles(packed, tiles, img):
    """Scatters one rank's packed tiles (as rt_render_tiles writes them) into img [ny, nx, 3]."""
    t = np.asarray(tiles, dtype=np.int64).reshape(-1, 4)
    if t.size and (t[:, 2:] == 1).all():   # pixel layouts: one vectorised scatter
        img[t[:, 1], t[:, 0]] = np.asarray(packed[: 3 * len(t)]).reshape(-1, 3)
        return img
    off = 0
    for x0, y0, w, h in tiles:
        img[y0:y0 + h, x0:x0 + w] = np.asarray(packed[off:off + w * h * 3]).reshape(h, w, 3)
        off += w * h * 3
    return img
