"""oracle/oracle.py — TEST INFRASTRUCTURE ONLY.

ctypes view of the plain-C restatement (liboracle.so, rt_oracle.h) and a runner
for the reference binary compiled from /root/reference (oracle/_ref/ref_render).
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")
REF_BIN = os.path.join(HERE, "_ref", "ref_render")

SCENES = {
    "random_scene": 0, "random_motion": 1, "cornell_box": 2, "cornell_smoke": 3,
    "final": 4, "simple_light": 5, "two_spheres": 6, "test": 7, "earth": 8,
    "edge_empty": 9, "edge_single": 10, "edge_degenerate": 11,   # the tests' edge cases (ref_harness.cpp edge_*)
    "edge_chains": 12,
}
EARTH_PNG = os.path.join(os.path.dirname(HERE), "tests", "golden", "picture.png")   # main.cpp:93's asset
CAMERAS = {"cornell": 0, "random": 1, "final_alt": 2}
# Per-scene defaults, as the reference driver pairs them (main.cpp:254-291) plus
# the chapter-1/3 sky background for the random scenes.
SCENE_DEFAULTS = {
    "random_scene": dict(camera="random", background="sky", max_depth=8),
    "random_motion": dict(camera="random", background="sky", max_depth=50),
    "cornell_box": dict(camera="cornell", background="black", max_depth=50),
    "cornell_smoke": dict(camera="cornell", background="black", max_depth=50),
    "final": dict(camera="cornell", background="black", max_depth=50),
    "simple_light": dict(camera="random", background="black", max_depth=50),
    "two_spheres": dict(camera="random", background="black", max_depth=50),
    "test": dict(camera="random", background="black", max_depth=50),
    "earth": dict(camera="cornell", background="black", max_depth=50),
    "edge_empty": dict(camera="random", background="sky", max_depth=50),
    "edge_single": dict(camera="random", background="sky", max_depth=50),
    "edge_degenerate": dict(camera="random", background="sky", max_depth=50),
    "edge_chains": dict(camera="random", background="sky", max_depth=50),
}


def host_libm_pinned():
    """(pinned, why): whether this host's libm is the one csrc/hip/rt_libm.h restates —
    glibc 2.35 on an x86-64 CPU with FMA (its sinf ifunc then runs the FMA variant whose
    constants rt_libm.h was read from).  The oracle calls the host's sinf / asinf / atan2f
    (texture.h:36, 55; hitable.h:14-19), so a GPU image is the oracle's bit for bit only on
    such a host; on another the parity bar is north_star's RMS one and the exact-pixel
    share is reported, not asserted (tests/test_gpu_parity.py assert_exact, smoke())."""
    import platform
    try:
        libc = ctypes.CDLL("libc.so.6")
        libc.gnu_get_libc_version.restype = ctypes.c_char_p
        ver = libc.gnu_get_libc_version().decode()
    except (OSError, AttributeError):
        return False, "the host C library is not glibc"
    if ver != "2.35":
        return False, f"host glibc {ver}, rt_libm.h restates 2.35"
    if platform.machine() != "x86_64":
        return False, f"host {platform.machine()}, rt_libm.h restates the x86-64 FMA variant"
    try:
        flags = open("/proc/cpuinfo").read()
    except OSError:
        return False, "no /proc/cpuinfo to check for FMA"
    if " fma" not in flags:
        return False, "host CPU without FMA: glibc's sinf runs its non-FMA variant"
    return True, "glibc 2.35, x86-64 with FMA"


def png_rgba(path):
    """Minimal 8-bit non-interlaced PNG decode (test-side; independent of the product's)."""
    import struct
    import zlib
    d = open(path, "rb").read()
    assert d[:8] == b"\x89PNG\r\n\x1a\n"
    i, idat, w, h, ct = 8, b"", 0, 0, 0
    while i < len(d):
        n, = struct.unpack(">I", d[i:i + 4])
        t = d[i + 4:i + 8]
        if t == b"IHDR":
            w, h, bd, ct = struct.unpack(">IIBB", d[i + 8:i + 18])
            assert bd == 8
        elif t == b"IDAT":
            idat += d[i + 8:i + 8 + n]
        i += 12 + n
    ch = {0: 1, 2: 3, 4: 2, 6: 4}[ct]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * ch + 1)
    out = np.zeros((h, w * ch), np.int32)
    for y in range(h):
        f, row = raw[y, 0], raw[y, 1:].astype(np.int32)
        up = out[y - 1] if y else np.zeros(w * ch, np.int32)
        cur = np.zeros(w * ch, np.int32)
        for x in range(w * ch):
            a = cur[x - ch] if x >= ch else 0
            b = up[x]
            c = up[x - ch] if x >= ch else 0
            if f == 0: v = row[x]
            elif f == 1: v = row[x] + a
            elif f == 2: v = row[x] + b
            elif f == 3: v = row[x] + ((a + b) >> 1)
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                v = row[x] + (a if pa <= pb and pa <= pc else (b if pb <= pc else c))
            cur[x] = v & 255
        out[y] = cur
    return out.astype(np.uint8).reshape(h, w, ch)


_image_loaded = False


def load_earth_image(path=None):
    """Hands earth()'s texels to the oracle (done once per process)."""
    global _image_loaded
    if _image_loaded:
        return
    img = np.ascontiguousarray(png_rgba(path or EARTH_PNG))
    h, w, ch = img.shape
    lib().oracle_set_image(img.ctypes.data, w, h, ch)
    _image_loaded = True


class OracleParams(ctypes.Structure):
    _fields_ = [
        ("scene", ctypes.c_int32), ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("ns", ctypes.c_int32),
        ("max_depth", ctypes.c_int32), ("background", ctypes.c_int32), ("tmin", ctypes.c_float),
        ("camera", ctypes.c_int32), ("rng", ctypes.c_int32), ("media_after", ctypes.c_int32),
        ("forward", ctypes.c_int32), ("chunk", ctypes.c_int32),
        ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
        ("threads", ctypes.c_int32), ("sample_offset", ctypes.c_uint32), ("pad_", ctypes.c_uint32),
        ("seed", ctypes.c_uint64),
    ]


class OracleStats(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_double), ("segments", ctypes.c_double), ("seconds", ctypes.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C oracle`")
        L = ctypes.CDLL(LIB_PATH)
        L.oracle_render.argtypes = [ctypes.POINTER(OracleParams), ctypes.c_void_p, ctypes.POINTER(OracleStats)]
        L.oracle_render.restype = ctypes.c_int
        L.oracle_quantize.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.oracle_ppm_text.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_long]
        L.oracle_ppm_text.restype = ctypes.c_long
        L.oracle_perlin_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.oracle_drand48.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
        L.oracle_counter_draws.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        L.oracle_medium_draw.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int]
        L.oracle_medium_draw.restype = ctypes.c_double
        L.oracle_render_axis.argtypes = [ctypes.POINTER(OracleParams), ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(OracleStats)]
        L.oracle_render_axis.restype = ctypes.c_int
        L.oracle_scene_dump.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_long]
        L.oracle_set_image.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.oracle_scene_dump.restype = ctypes.c_long
        L.oracle_render_desc.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(OracleParams), ctypes.c_void_p,
                                         ctypes.POINTER(OracleStats)]
        L.oracle_render_desc.restype = ctypes.c_int
        L.oracle_first_hits_desc.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(OracleParams)] + \
            [ctypes.c_void_p] * 4
        L.oracle_first_hits_desc.restype = ctypes.c_int
        L.oracle_trace_rays_desc.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + \
            [ctypes.c_void_p] * 5
        L.oracle_trace_rays.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 5
        L.oracle_radiance_rays_desc.argtypes = [ctypes.c_void_p, ctypes.POINTER(OracleParams), ctypes.c_void_p,
                                                ctypes.c_int64, ctypes.c_void_p]
        L.oracle_radiance_rays.argtypes = [ctypes.POINTER(OracleParams), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        for f in (L.oracle_trace_rays_desc, L.oracle_trace_rays, L.oracle_radiance_rays_desc, L.oracle_radiance_rays):
            f.restype = ctypes.c_int
        _lib = L
    return _lib


@dataclass
class RenderSpec:
    scene: str = "final"
    nx: int = 40
    ny: int = 40
    ns: int = 4
    max_depth: int | None = None
    background: str | None = None
    camera: str | None = None
    tmin: float = 0.001
    rng: str = "canonical"          # or "counter"
    seed: int = 0
    sample_offset: int = 0
    media_after: bool = False       # kernel order
    forward: bool = False           # kernel accumulation
    chunk: int = 0
    rect: tuple | None = None       # (x0, y0, w, h) image coords
    threads: int = 1

    def resolved(self):
        d = SCENE_DEFAULTS[self.scene]
        return (self.max_depth if self.max_depth is not None else d["max_depth"],
                self.background or d["background"], self.camera or d["camera"])


def render(spec: RenderSpec, axis=None):
    """Returns (mean float32 array [h, w, 3], stats dict).  axis: a uint8 array [h, w] that
    receives 1 where a pixel's paths traced a ray with a direction component of exactly 0
    (oracle_render_axis)."""
    if spec.scene == "earth":
        load_earth_image()
    depth, bg, cam = spec.resolved()
    x0, y0, w, h = spec.rect if spec.rect else (0, 0, spec.nx, spec.ny)
    p = OracleParams(scene=SCENES[spec.scene], nx=spec.nx, ny=spec.ny, ns=spec.ns, max_depth=depth,
                     background=1 if bg == "sky" else 0, tmin=spec.tmin, camera=CAMERAS[cam],
                     rng=1 if spec.rng == "counter" else 0, media_after=int(spec.media_after),
                     forward=int(spec.forward), chunk=spec.chunk, x0=x0, y0=y0, w=w, h=h,
                     threads=spec.threads, sample_offset=spec.sample_offset, seed=spec.seed)
    out = np.zeros((h, w, 3), dtype=np.float32)
    st = OracleStats()
    if axis is not None:
        assert axis.dtype == np.uint8 and axis.shape == (h, w) and axis.flags.c_contiguous
    rc = lib().oracle_render_axis(ctypes.byref(p), out.ctypes.data, None if axis is None else axis.ctypes.data,
                                  ctypes.byref(st))
    if rc != 0:
        raise RuntimeError(f"oracle_render failed: {rc}")
    return out, {"samples": st.samples, "segments": st.segments, "seconds": st.seconds}


def kernel_spec(scene: str, nx: int, ny: int, ns: int, *, seed: int = 0, chunk: int = 0, **kw) -> RenderSpec:
    """The CPU statement of exactly what the GPU kernel computes (counter RNG,
    media after surfaces, forward throughput, chunked partial sums)."""
    return RenderSpec(scene=scene, nx=nx, ny=ny, ns=ns, rng="counter", seed=seed, media_after=True,
                      forward=True, chunk=chunk, **kw)


def _desc_params(spec: RenderSpec):
    """oracle_params of a descriptor render: spec.scene and spec.camera are not used, the depth
    and background must be given."""
    if spec.max_depth is None or spec.background is None:
        raise ValueError("a descriptor render needs max_depth and background")
    if spec.rng != "counter":
        raise ValueError("a descriptor render uses the counter RNG")
    x0, y0, w, h = spec.rect if spec.rect else (0, 0, spec.nx, spec.ny)
    p = OracleParams(scene=-1, nx=spec.nx, ny=spec.ny, ns=spec.ns, max_depth=spec.max_depth,
                     background=1 if spec.background == "sky" else 0, tmin=spec.tmin, camera=0, rng=1,
                     media_after=int(spec.media_after), forward=int(spec.forward), chunk=spec.chunk,
                     x0=x0, y0=y0, w=w, h=h, threads=spec.threads, sample_offset=spec.sample_offset, seed=spec.seed)
    return p, w, h


def _desc_pointers(desc, cam):
    """Addresses of an rtnw.SceneDesc's rt_scene_desc and an rtnw.Camera's rt_camera_desc."""
    return ctypes.cast(desc.ptr, ctypes.c_void_p), ctypes.cast(ctypes.pointer(cam.desc), ctypes.c_void_p)


def desc_spec(nx: int, ny: int, ns: int, *, max_depth: int, background: str, seed: int = 0, chunk: int = 0,
              forward: bool = True, media_after: bool = True, **kw) -> RenderSpec:
    """The spec of a descriptor render: kernel_spec's statement by default (forward=False is
    the right-fold mode RT_FLAG_RIGHT_FOLD implements)."""
    return RenderSpec(scene="", nx=nx, ny=ny, ns=ns, rng="counter", seed=seed, media_after=media_after,
                      forward=forward, chunk=chunk, max_depth=max_depth, background=background, **kw)


def render_desc(desc, cam, spec: RenderSpec):
    """oracle_render_desc: the oracle's image of any rtnw.SceneDesc through an rtnw.Camera.
    Returns (mean float32 array [h, w, 3], stats dict)."""
    p, w, h = _desc_params(spec)
    dp, cp = _desc_pointers(desc, cam)
    out = np.zeros((h, w, 3), dtype=np.float32)
    st = OracleStats()
    rc = lib().oracle_render_desc(dp, cp, ctypes.byref(p), out.ctypes.data, ctypes.byref(st))
    if rc != 0:
        raise RuntimeError(f"oracle_render_desc failed: {rc}")
    return out, {"samples": st.samples, "segments": st.segments, "seconds": st.seconds}


def first_hits_desc(desc, cam, spec: RenderSpec):
    """oracle_first_hits_desc: per camera sample the first surface hit, media skipped.  A dict
    of prim [h, w, ns] int32 (-1: miss), hit [h, w, ns] bool, depth [h, w, ns], normal and
    albedo [h, w, ns, 3], float32."""
    p, w, h = _desc_params(spec)
    dp, cp = _desc_pointers(desc, cam)
    prim = np.zeros((h, w, spec.ns), np.int32)
    depth = np.zeros((h, w, spec.ns), np.float32)
    normal = np.zeros((h, w, spec.ns, 3), np.float32)
    albedo = np.zeros((h, w, spec.ns, 3), np.float32)
    rc = lib().oracle_first_hits_desc(dp, cp, ctypes.byref(p), prim.ctypes.data, depth.ctypes.data, normal.ctypes.data,
                                      albedo.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"oracle_first_hits_desc failed: {rc}")
    return dict(prim=prim, hit=prim >= 0, depth=depth, normal=normal, albedo=albedo)


# rt_ray, rt_path_ray and rt_radiance as numpy records (include/rt_hip.h; the layouts of rtnw's)
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("dir", np.float32, 3), ("t_max", np.float32),
                      ("time", np.float32), ("pad", np.float32, 3)])
PATH_RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("time", np.float32), ("dir", np.float32, 3), ("skip", np.uint32),
                           ("pixel", np.uint32), ("sample", np.uint32), ("pad", np.uint32, 2)])
RADIANCE_DTYPE = np.dtype([("rgb", np.float32, 3), ("status", np.int32)])


def _records(rays, dtype):
    r = np.ascontiguousarray(rays)
    if r.dtype != dtype:
        raise TypeError(f"rays must be records of {dtype.names}")
    return r.reshape(-1)


def _trace(call, r, threads, materials):
    n = len(r)
    prim, t, depth = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    normal, albedo = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    rc = call(r.ctypes.data, n, threads, prim.ctypes.data, t.ctypes.data, depth.ctypes.data, normal.ctypes.data,
              albedo.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"oracle trace_rays failed: {rc}")
    material = np.full(n, -1, np.int32) if materials is None else np.append(materials, -1).astype(np.int32)[prim]
    return dict(prim=prim, material=material, t=t, depth=depth, normal=normal, albedo=albedo, pad=np.zeros((n, 2), np.int32))


def trace_rays_desc(desc, rays, threads: int = 1):
    """oracle_trace_rays_desc: the closest surface hit of each rt_ray record (rtnw.pack_rays) in
    an rtnw.SceneDesc, media skipped, as the dict rtnw.Scene.trace_rays returns: prim (-1: miss),
    material (the descriptor's, -1 on a miss) [n] int32, t, depth [n], normal, albedo [n, 3]
    float32, pad [n, 2] zeros.  Valid rays only: no validity rule is restated."""
    c = desc.contents
    mats = np.array([c.prims[i].material for i in range(c.nprims)], np.int32)
    dp = ctypes.cast(desc.ptr, ctypes.c_void_p)
    return _trace(lambda *a: lib().oracle_trace_rays_desc(dp, *a), _records(rays, RAY_DTYPE), threads, mats)


def trace_rays(scene: str, rays, threads: int = 1):
    """oracle_trace_rays: the same over a built-in scene; prim is the leaf's place in list order
    (depth first, media left out) and material is -1 throughout."""
    if scene == "earth":
        load_earth_image()
    return _trace(lambda *a: lib().oracle_trace_rays(SCENES[scene], *a), _records(rays, RAY_DTYPE), threads, None)


def _ray_params(scene, max_depth, background, seed, tmin, forward, media_after, threads):
    return OracleParams(scene=scene, nx=1, ny=1, ns=1, max_depth=max_depth, background=1 if background == "sky" else 0,
                        tmin=tmin, camera=0, rng=1, media_after=int(media_after), forward=int(forward), threads=threads,
                        seed=seed)


def _radiance(call, r):
    out = np.zeros(len(r), RADIANCE_DTYPE)
    rgb = np.zeros((len(r), 3), np.float32)
    rc = call(r.ctypes.data, len(r), rgb.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"oracle radiance_rays failed: {rc}")
    out["rgb"] = rgb
    return out


def radiance_rays_desc(desc, rays, *, max_depth: int, background: str, seed: int = 0, tmin: float = 0.001,
                       forward: bool = True, media_after: bool = True, threads: int = 1):
    """oracle_radiance_rays_desc: 0 + de_nan(color()) of each rt_path_ray record
    (rtnw.pack_path_rays) in an rtnw.SceneDesc as [n] records like rtnw.Scene.radiance_rays'
    (rgb [n, 3] float32, status 0): the kernel's statement by default, the reference's order with
    forward=False, media_after=False.  Valid rays only."""
    p = _ray_params(-1, max_depth, background, seed, tmin, forward, media_after, threads)
    dp = ctypes.cast(desc.ptr, ctypes.c_void_p)
    return _radiance(lambda *a: lib().oracle_radiance_rays_desc(dp, ctypes.byref(p), *a), _records(rays, PATH_RAY_DTYPE))


def radiance_rays(scene: str, rays, *, max_depth: int, background: str, seed: int = 0, tmin: float = 0.001,
                  forward: bool = True, media_after: bool = True, threads: int = 1):
    """oracle_radiance_rays: the same over a built-in scene."""
    if scene == "earth":
        load_earth_image()
    p = _ray_params(SCENES[scene], max_depth, background, seed, tmin, forward, media_after, threads)
    return _radiance(lambda *a: lib().oracle_radiance_rays(ctypes.byref(p), *a), _records(rays, PATH_RAY_DTYPE))


def feature_means(fh):
    """What rt_render_features writes for those samples: each buffer's samples added in sample
    order in float32, the sum times float(1.0 / spp).  albedo, normal [h, w, 3]; depth,
    coverage [h, w]."""
    ns = fh["prim"].shape[-1]
    k = np.float32(1.0 / ns)

    def mean(a):   # [h, w, ns, ...] -> [h, w, ...]
        acc = np.zeros(a.shape[:2] + a.shape[3:], np.float32)
        for s in range(ns):
            acc = acc + a[:, :, s]
        return acc * k
    return dict(albedo=mean(fh["albedo"]), normal=mean(fh["normal"]), depth=mean(fh["depth"]),
                coverage=mean(fh["hit"].astype(np.float32)))


def quantize(mean: np.ndarray) -> np.ndarray:
    m = np.ascontiguousarray(mean, dtype=np.float32)
    n = m.size // 3
    rgb = np.zeros(n * 3, dtype=np.uint8)
    lib().oracle_quantize(m.ctypes.data, n, rgb.ctypes.data)
    return rgb.reshape(m.shape)


def ppm_text(rgb: np.ndarray) -> bytes:
    h, w, _ = rgb.shape
    r = np.ascontiguousarray(rgb, dtype=np.uint8)
    n = lib().oracle_ppm_text(r.ctypes.data, w, h, None, 0)
    buf = ctypes.create_string_buffer(n)
    lib().oracle_ppm_text(r.ctypes.data, w, h, buf, n)
    return buf.raw[:n]


def ppm_md5(mean: np.ndarray) -> str:
    return hashlib.md5(ppm_text(quantize(mean))).hexdigest()


def perlin_tables():
    rv = np.zeros(768, dtype=np.float32)
    pm = np.zeros(768, dtype=np.int32)
    lib().oracle_perlin_tables(rv.ctypes.data, pm.ctypes.data)
    return rv.reshape(256, 3), pm.reshape(3, 256)


def drand48_stream(x0: int, n: int) -> np.ndarray:
    out = np.zeros(n, dtype=np.float64)
    lib().oracle_drand48(x0, n, out.ctypes.data)
    return out


def counter_draws(seed: int, pixel: int, sample: int, n: int) -> np.ndarray:
    out = np.zeros(n, dtype=np.float64)
    lib().oracle_counter_draws(seed, pixel, sample, n, out.ctypes.data)
    return out


def medium_draw(seed: int, pixel: int, sample: int, bounce: int, medium: int, nmedia: int) -> float:
    """constant_medium draw of medium `medium` at segment `bounce` in a scene of `nmedia` media."""
    return lib().oracle_medium_draw(seed, pixel, sample, bounce, medium, nmedia)


def scene_dump(scene: str) -> str:
    if scene == "earth":
        load_earth_image()
    n = lib().oracle_scene_dump(SCENES[scene], None, 0)
    buf = ctypes.create_string_buffer(n)
    lib().oracle_scene_dump(SCENES[scene], buf, n)
    return buf.raw[:n].decode()


# ------------------------------------------------------------ reference binary
def have_ref() -> bool:
    return os.path.exists(REF_BIN) and os.access(REF_BIN, os.X_OK)


def ref_render(spec: RenderSpec, workdir: str, rows: tuple | None = None, timing: bool = False):
    """Runs the compiled reference; returns (mean [rows, nx, 3], ppm bytes, timing dict|None)."""
    depth, bg, cam = spec.resolved()
    fb = os.path.join(workdir, "ref_fb.f32")
    ppm = os.path.join(workdir, "ref.ppm")
    cmd = [REF_BIN, "--scene", spec.scene, "--nx", str(spec.nx), "--ny", str(spec.ny), "--ns", str(spec.ns),
           "--depth", str(depth), "--bg", bg, "--cam", cam, "--tmin", repr(spec.tmin),
           "--rng", spec.rng, "--seed", str(spec.seed), "--fb", fb, "--ppm", ppm,
           "--assets", os.path.dirname(EARTH_PNG)]
    if rows:
        cmd += ["--rows", f"{rows[0]}:{rows[1]}"]
    if timing:
        cmd += ["--time"]
    res = subprocess.run(cmd, capture_output=True, text=True, check=True)
    nrows = (rows[1] - rows[0]) if rows else spec.ny
    mean = np.fromfile(fb, dtype=np.float32).reshape(nrows, spec.nx, 3)
    with open(ppm, "rb") as f:
        text = f.read()
    tinfo = None
    if timing:
        import json
        tinfo = json.loads(res.stdout.strip().splitlines()[-1])
    return mean, text, tinfo


_ref_rays = None


def have_ref_rays() -> bool:
    """Whether the reference binary is there and has the ray mode (ref_harness.cpp --rays,
    --path-rays).  oracle/_ref is not in git: where the reference tree is absent `make -C oracle`
    rebuilds nothing and a binary kept from an earlier build, which may predate the mode, is what
    runs.  Asked of the binary by having it do the job on no records: a binary with the mode
    reads an empty file, writes an empty one and exits 0; one without it ends in usage() (2)."""
    global _ref_rays
    if _ref_rays is None:
        _ref_rays = False
        if have_ref():
            try:
                res = subprocess.run([REF_BIN, "--scene", "edge_single", "--rays", os.devnull, "--hits", os.devnull,
                                      "--path-rays", os.devnull, "--radiance", os.devnull], capture_output=True, timeout=60)
                _ref_rays = res.returncode == 0
            except (OSError, subprocess.TimeoutExpired):
                pass
    return _ref_rays


REF_HIT_FIELDS = 9   # the harness's answer per ray: hit (0 or 1), t, depth, normal[3], albedo[3]


def ref_trace_rays(scene: str, rays, workdir: str) -> np.ndarray:
    """The compiled reference's own world->hit on each rt_ray record: [n, 9] float32 of hit, t,
    depth, normal, albedo (a miss: zeros and an albedo of 1, as the oracle reports it)."""
    r = _records(rays, RAY_DTYPE)
    src, dst = os.path.join(workdir, "rays.bin"), os.path.join(workdir, "hits.f32")
    r.tofile(src)
    subprocess.run([REF_BIN, "--scene", scene, "--rays", src, "--hits", dst, "--assets", os.path.dirname(EARTH_PNG)],
                   capture_output=True, check=True)
    return np.fromfile(dst, dtype=np.float32).reshape(len(r), REF_HIT_FIELDS)


def ref_radiance_rays(scene: str, rays, workdir: str, *, max_depth: int, background: str, seed: int = 0,
                      tmin: float = 0.001) -> np.ndarray:
    """The compiled reference's own color() on each rt_path_ray record, the counter stream
    restarted at the record's key and advanced by its skip: [n, 3] float32."""
    r = _records(rays, PATH_RAY_DTYPE)
    src, dst = os.path.join(workdir, "path_rays.bin"), os.path.join(workdir, "radiance.f32")
    r.tofile(src)
    subprocess.run([REF_BIN, "--scene", scene, "--path-rays", src, "--radiance", dst, "--seed", str(seed),
                    "--depth", str(max_depth), "--bg", background, "--tmin", repr(tmin),
                    "--assets", os.path.dirname(EARTH_PNG)], capture_output=True, check=True)
    return np.fromfile(dst, dtype=np.float32).reshape(len(r), 3)


def ref_dump(scene: str, workdir: str) -> str:
    path = os.path.join(workdir, f"dump_{scene}.txt")
    subprocess.run([REF_BIN, "--scene", scene, "--nx", "1", "--ny", "1", "--ns", "1", "--dump", path,
                    "--assets", os.path.dirname(EARTH_PNG)],
                   capture_output=True, check=True)
    with open(path) as f:
        return f.read()
