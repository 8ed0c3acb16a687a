#!/usr/bin/env python3
"""tools/radiance_probe.py — what radiance queries cost (rt_radiance_rays), and a
picture no camera of the library can take.

1. Rates.  For final() and random_scene at 500 x 500 it restates the camera's own samples
   0 .. --spp - 1 of every pixel as rt_path_ray records (the drand48 streams of DESIGN.md §3 in
   numpy: jitter, lens-disk rejection, time draw; the records' skip is the draws spent), checks
   that rt_radiance_rays returns rt_render_tile's samples bit for bit (the ray-tracing identity
   of rt_hip.h, here at the size that is timed), and then times

     query    rt_radiance_rays_dev on the records in device memory (the RT_FEAT_ALL ray-source
              variant; 48 B read and 16 B written per sample), and
     render   rt_render_tiles on the same samples (chunk 1: the scene's specialised variant, 12 B
              of slab per sample, and the resolve kernel behind it; its kernel_ms is the
              megakernel alone).

   Method: each figure is the wall time of --reps back-to-back enqueues on the default stream
   ended by a device synchronise, over --reps; the two take turns, --rounds rounds each after one
   warm-up round; median and span are reported, with the render's HIP-event kernel time.

2. The demonstration.  A lat-long panorama of final() from a point among its objects: --pano-width x
   --pano-width / 2 directions over the whole sphere, --pano-spp samples each (stream keys: the
   panorama's own pixel numbers), averaged and written to <out>/panorama_final.npy
   ([h, w, 3] float32, linear radiance).

Writes <out>/radiance_probe.json and <out>/radiance_probe.md.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "peter-shirley-ray-tracing-the-next-week_amd"))
import rtnw  # noqa: E402

SCENES = {"final": "cornell", "random_scene": "random"}
NX = NY = 500
M48 = np.uint64(0xFFFFFFFFFFFF)


# ------------------------------------------------------------------ the sample streams in numpy
def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def lcg(x):
    return (x * np.uint64(0x5DEECE66D) + np.uint64(0xB)) & M48


def draw(x):
    return x.astype(np.float64) * 2.0 ** -48


def camera_records(cam, nx, ny, spp, seed):
    """Every camera sample of the frame (camera.h:41-56 after main.cpp:305-306) as rt_path_ray
    records, in (row, column, sample) order, row 0 the image's top row."""
    d = cam.desc
    f = np.float32
    llc, hor, ver, org, cu, cv = (np.array(list(v), f) for v in (d.lower_left_corner, d.horizontal, d.vertical, d.origin,
                                                                 d.u, d.v))
    row, col, smp = (a.reshape(-1) for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(spp), indexing="ij"))
    j = ny - 1 - row
    pix = (j * nx + col).astype(np.uint64)
    with np.errstate(over="ignore"):
        skey = mix64(np.uint64(seed) ^ np.uint64(0x5851F42D4C957F2D))
        x = mix64(skey ^ ((pix << np.uint64(32)) | smp.astype(np.uint64))) & M48
        x = lcg(x)
        s = ((col + draw(x)).astype(f) / f(nx)).reshape(-1, 1)
        x = lcg(x)
        t = ((j + draw(x)).astype(f) / f(ny)).reshape(-1, 1)
        n = len(pix)
        px, py = np.zeros(n, f), np.zeros(n, f)
        skip = np.full(n, 2, np.uint32)
        todo = np.ones(n, bool)
        while todo.any():           # do ... while (dot(p, p) >= 1.0), camera.h:6-12
            x1 = lcg(x)
            x2 = lcg(x1)
            cx, cy = f(2.0) * draw(x1).astype(f) - f(1), f(2.0) * draw(x2).astype(f) - f(1)
            px, py = np.where(todo, cx, px), np.where(todo, cy, py)
            x = np.where(todo, x2, x)
            skip = skip + todo.astype(np.uint32) * np.uint32(2)
            todo = todo & ~((px * px + py * py) + f(0) < f(1))
        x = lcg(x)
    tm = (np.float64(f(d.time0)) + draw(x) * np.float64(f(d.time1) - f(d.time0))).astype(f)
    skip = skip + np.uint32(1)
    lens = f(d.lens_radius)
    offset = cu * (lens * px).reshape(-1, 1) + cv * (lens * py).reshape(-1, 1)
    dirs = (((llc + s * hor) + t * ver) - org) - offset
    assert dirs.dtype == f and int(skip.max()) <= rtnw.RT_RADIANCE_MAX_SKIP
    return rtnw.pack_path_rays(org + offset, dirs, tm, pix.astype(np.uint32), smp.astype(np.uint32), skip)


# ------------------------------------------------------------------ 1. rates
def timed(enqueue, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        enqueue()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def summary(ms, n):
    med = statistics.median(ms)
    return dict(ms=med, ms_min=min(ms), ms_max=max(ms), msamples_per_s=n / med / 1e3)


def probe_scene(name, args):
    import torch
    _, bg, depth = rtnw.SCENE_DEFAULTS[name]
    scene = rtnw.Scene.builtin(name)
    cam = rtnw.Camera.preset(SCENES[name], NX, NY)
    spp = args.spp
    rays = camera_records(cam, NX, NY, spp, args.seed)
    n = len(rays)
    q = rtnw.RenderParams(1, 1, 1, max_depth=depth, background=bg, seed=args.seed)
    # the identity at the timed size: every sample of the frame against the render's
    scene.radiance_rays(q, rays[:4096])    # (the first launch loads the code object)
    rec, host_ms = scene.radiance_rays(q, rays, timing=True)
    rgb = rec["rgb"].reshape(NY, NX, spp, 3)
    identical = bool((rec["status"] == 0).all())
    for s in range(spp):
        p1 = rtnw.RenderParams(NX, NY, 1, max_depth=depth, background=bg, chunk=1, seed=args.seed, sample_offset=s)
        img = scene.render_tile(cam, p1, 0, 0, NX, NY)
        identical = identical and np.array_equal(rgb[:, :, s].view(np.uint32), img.view(np.uint32))
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    d_rec = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_img = torch.zeros(NY * NX * 3, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = rtnw.RenderParams(NX, NY, spp, max_depth=depth, background=bg, chunk=1, seed=args.seed)
    kernel_ms = []

    def query():
        scene.radiance_rays_dev(q, d_rays.data_ptr(), n, d_rec.data_ptr(), stream)

    def render():
        scene.render_tiles(cam, p, [(0, 0, NX, NY)], d_img.data_ptr(), stream, stats=False)

    ms = dict(query=[], render=[])
    for r in range(args.rounds + 1):   # round 0 warms up; the two take turns
        for k, fn in (("query", query), ("render", render)):
            t = timed(fn, args.reps)
            if r:
                ms[k].append(t)
        st = scene.render_tiles(cam, p, [(0, 0, NX, NY)], d_img.data_ptr(), stream, stats=True)
        if r:
            kernel_ms.append(st["kernel_ms"])
    out = dict(scene=name, samples=n, spp=spp, identical_to_render=identical, host_form_kernel_ms=host_ms,
               query=summary(ms["query"], n), render=summary(ms["render"], n),
               render_kernel_ms=statistics.median(kernel_ms))
    out["query_over_render"] = out["query"]["ms"] / out["render"]["ms"]
    out["query_over_render_kernel"] = out["query"]["ms"] / out["render_kernel_ms"]
    scene.close()
    return out


# ------------------------------------------------------------------ 2. the panorama
def panorama(args):
    scene = rtnw.Scene.builtin("final")
    _, bg, depth = rtnw.SCENE_DEFAULTS["final"]
    w, h, spp = args.pano_width, args.pano_width // 2, args.pano_spp
    f = np.float32
    row, col, smp = (a.reshape(-1) for a in np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij"))
    pix = (row * w + col).astype(np.uint32)
    # each sample's direction is jittered inside its cell (numpy's generator: not the sample's stream)
    rng = np.random.default_rng(args.seed)
    u = (col + rng.random(len(col))) / w
    v = (row + rng.random(len(row))) / h
    phi, theta = 2 * np.pi * u, np.pi * v
    dirs = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], axis=1).astype(f)
    eye = np.array(args.pano_eye, f)
    rays = rtnw.pack_path_rays(eye, dirs, 0.0, pix, smp.astype(np.uint32), 0)
    q = rtnw.RenderParams(1, 1, 1, max_depth=depth, background=bg, seed=args.seed)
    rec, ms = scene.radiance_rays(q, rays, timing=True)
    assert (rec["status"] == 0).all()
    img = rec["rgb"].reshape(h, w, spp, 3).astype(np.float64).mean(axis=2).astype(f)
    path = os.path.join(args.out, "panorama_final.npy")
    np.save(path, img)
    scene.close()
    return dict(path=path, shape=list(img.shape), eye=list(map(float, eye)), spp=spp, rays=len(rays), kernel_ms=ms,
                mean=float(img.mean()), lit_share=float((img.sum(axis=-1) > 0).mean()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="radiance_probe_out")
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--pano-width", type=int, default=1024)
    ap.add_argument("--pano-spp", type=int, default=16)
    ap.add_argument("--pano-eye", type=float, nargs=3, default=(278.0, 278.0, 100.0))
    ap.add_argument("--no-panorama", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if rtnw.device_count() < 1:
        sys.exit("radiance_probe: no GPU (there is no CPU path to time)")
    res = dict(lib=rtnw.LIB_PATH, version=rtnw.lib().rt_version().decode(), nx=NX, ny=NY, rounds=args.rounds, reps=args.reps,
               scenes=[probe_scene(s, args) for s in args.scenes.split(",") if s])
    if not args.no_panorama:
        res["panorama"] = panorama(args)
    with open(os.path.join(args.out, "radiance_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = [f"# radiance_probe: {NX} x {NY} x spp samples per call, median of {args.rounds} rounds of {args.reps} calls (min - max)",
             "", "| scene | samples | identical to the render | query ms | Msamples/s | render ms | Msamples/s | render kernel ms |"
             " query / render | query / render kernel | host-form kernel ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for s in res["scenes"]:
        cell = lambda k: f"{s[k]['ms']:.3f} ({s[k]['ms_min']:.3f} - {s[k]['ms_max']:.3f}) | {s[k]['msamples_per_s']:.1f}"  # noqa: E731
        lines.append(f"| {s['scene']} | {s['samples']} | {s['identical_to_render']} | {cell('query')} | {cell('render')} | "
                     f"{s['render_kernel_ms']:.3f} | {s['query_over_render']:.3f} | {s['query_over_render_kernel']:.3f} | "
                     f"{s['host_form_kernel_ms']:.3f} |")
    if "panorama" in res:
        q = res["panorama"]
        lines += ["", f"panorama: {q['path']} shape {q['shape']} from {q['eye']}, {q['spp']} spp, {q['rays']} rays in "
                      f"{q['kernel_ms']:.2f} ms of kernel time; mean {q['mean']:.4f}, lit share {q['lit_share']:.3f}"]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(args.out, "radiance_probe.md"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
