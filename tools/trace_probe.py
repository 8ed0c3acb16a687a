#!/usr/bin/env python3
"""tools/trace_probe.py — what the ray queries cost (rt_trace_rays, rt_occluded).

For final(), random_scene and cornell_box at 500 x 500 it traces two ray sets of 250 000 rays,

  coherent     the camera's rays through the pixel centres (a pinhole at the camera's origin:
               the rays the feature pass traces at 1 spp, less its jitter and lens offset),
  incoherent   the same origins with directions drawn uniformly on the sphere
               (np.random.default_rng(--seed)),

with t_min 0.001, t_max +inf and, for both sets, times drawn uniformly in the scene's span, and
reports per scene and set the time per call and the Mrays/s of the closest-hit and the occlusion
query on device buffers (rt_trace_rays_dev, rt_occluded_dev: the kernels alone, 96 B and 49 B of
ray and result traffic per ray), the share of rays that hit, and the HIP-event kernel time the
host form reports for one batch.  The yardstick is the feature pass at spp = 1 on the same frame
(rt_render_features_dev: the same search from camera_ray(), 32 B of slab per sample and the
resolve kernel behind it).

Method: each figure is the wall time of --reps back-to-back enqueues on the default stream, ended
by a 4-byte copy back (a device synchronise), over --reps; the three entry points take turns,
--rounds rounds each after one warm-up round, and the median and the span are reported.
--scenes and --sets narrow the run: one scene and one set under `rocprofv3 --kernel-trace` gives
each kernel's own duration (profiles/r15/kernel_durations.txt).  --features-only measures the
yardstick alone: run it with RTNW_LIB pointing at another build of the library (the parent
commit's) to record that library's feature pass beside this one's.

Writes <out>/trace_probe.json and <out>/trace_probe.md.  Not run by any test.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "peter-shirley-ray-tracing-the-next-week_amd"))
import rtnw  # noqa: E402

SCENES = {"final": "cornell", "random_scene": "random", "cornell_box": "cornell"}
NX = NY = 500


def camera_rays(cam):
    """Pinhole rays through the pixel centres, row 0 the image's top row."""
    d = cam.desc
    f = np.float32
    llc, hor, ver, org = (np.array(list(v), f) for v in (d.lower_left_corner, d.horizontal, d.vertical, d.origin))
    i, row = np.meshgrid(np.arange(NX), np.arange(NY))
    u = ((i + 0.5) / NX).astype(f).reshape(-1, 1)
    v = ((NY - 1 - row + 0.5) / NY).astype(f).reshape(-1, 1)
    dirs = ((llc + u * hor) + v * ver) - org
    return np.broadcast_to(org, dirs.shape).copy(), dirs


def sphere_dirs(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


class DeviceBuffer:
    def __init__(self, nbytes):
        self.p = ctypes.c_void_p()
        rtnw._check(rtnw.lib().rt_device_alloc(0, nbytes, ctypes.byref(self.p)))

    def free(self):
        rtnw.lib().rt_device_free(self.p)


def timed(enqueue, sync_src, reps):
    """ms per call of `reps` enqueues, ended by a 4-byte copy from sync_src."""
    word = np.zeros(1, np.uint32)
    t0 = time.perf_counter()
    for _ in range(reps):
        enqueue()
    rtnw._check(rtnw.lib().rt_copy_to_host(word.ctypes.data, sync_src, 4))
    return (time.perf_counter() - t0) * 1e3 / reps


def summary(ms, n):
    med = statistics.median(ms)
    return dict(ms=med, ms_min=min(ms), ms_max=max(ms), mrays_per_s=n / med / 1e3)


def probe_scene(name, args):
    scene = rtnw.Scene.builtin(name)
    cam = rtnw.Camera.preset(SCENES[name], NX, NY)
    n = NX * NY
    params = rtnw.RenderParams(NX, NY, 1, seed=args.seed)
    guides = DeviceBuffer(n * 32)
    out = dict(scene=name, rays=n, sets={})

    def features():
        scene.render_features_dev(cam, params, 0, 0, NX, NY, guides.p.value)
    feat = []
    if args.features_only:
        for r in range(args.rounds + 1):
            ms = timed(features, guides.p, args.reps)
            if r:
                feat.append(ms)
        out["features"] = summary(feat, n)
        guides.free()
        scene.close()
        return out

    c = scene.desc.contents
    o, d = camera_rays(cam)
    times = np.random.default_rng(args.seed + 1).uniform(c.time0, c.time1, n).astype(np.float32)
    sets = {"coherent": d, "incoherent": sphere_dirs(n, args.seed)}
    sets = {k: v for k, v in sets.items() if k in args.sets.split(",")}
    rays_dev, hits_dev, occ_dev = DeviceBuffer(n * 48), DeviceBuffer(n * 48), DeviceBuffer(n)
    for label, dirs in sets.items():
        rays = rtnw.pack_rays(o, dirs, 0.001, np.inf, times)
        hit, host_trace_ms = scene.trace_rays(rays, timing=True)
        occ, host_occ_ms = scene.occluded(rays, timing=True)
        assert np.array_equal(occ, (hit["prim"] >= 0).astype(np.uint8))
        rtnw._check(rtnw.lib().rt_copy_to_device(rays_dev.p, rays.ctypes.data, rays.nbytes))
        calls = {"trace": lambda: scene.trace_rays_dev(rays_dev.p.value, n, hits_dev.p.value),
                 "occluded": lambda: scene.occluded_dev(rays_dev.p.value, n, occ_dev.p.value),
                 "features": features}
        sync = {"trace": hits_dev.p, "occluded": occ_dev.p, "features": guides.p}
        ms = {k: [] for k in calls}
        for r in range(args.rounds + 1):   # round 0 warms up; the entry points take turns
            for k, fn in calls.items():
                t = timed(fn, sync[k], args.reps)
                if r:
                    ms[k].append(t)
        out["sets"][label] = dict(hit_share=float(np.mean(hit["prim"] >= 0)), host_trace_kernel_ms=host_trace_ms,
                                  host_occluded_kernel_ms=host_occ_ms, **{k: summary(v, n) for k, v in ms.items()})
    for b in (rays_dev, hits_dev, occ_dev, guides):
        b.free()
    scene.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="trace_probe_out")
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--sets", default="coherent,incoherent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--features-only", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if rtnw.device_count() < 1:
        sys.exit("trace_probe: no GPU (there is no CPU path to time)")
    res = dict(lib=rtnw.LIB_PATH, version=rtnw.lib().rt_version().decode(), nx=NX, ny=NY, rounds=args.rounds, reps=args.reps,
               scenes=[probe_scene(s, args) for s in args.scenes.split(",")])
    stem = "trace_probe_features" if args.features_only else "trace_probe"
    with open(os.path.join(args.out, stem + ".json"), "w") as f:
        json.dump(res, f, indent=1)
    lines = [f"# {stem}: {NX} x {NY} rays per call, median of {args.rounds} rounds of {args.reps} calls (min - max)", ""]
    if args.features_only:
        lines += ["| scene | feature pass ms | Mrays/s |", "|---|---|---|"]
        for s in res["scenes"]:
            q = s["features"]
            lines.append(f"| {s['scene']} | {q['ms']:.4f} ({q['ms_min']:.4f} - {q['ms_max']:.4f}) | {q['mrays_per_s']:.0f} |")
    else:
        lines += ["| scene | rays | hit share | closest hit ms | Mrays/s | occlusion ms | Mrays/s | feature pass ms | Mrays/s |"
                  " host-form kernel ms (closest, occlusion) |", "|---|---|---|---|---|---|---|---|---|---|"]
        for s in res["scenes"]:
            for label, q in s["sets"].items():
                cell = lambda k: f"{q[k]['ms']:.4f} ({q[k]['ms_min']:.4f} - {q[k]['ms_max']:.4f}) | {q[k]['mrays_per_s']:.0f}"  # noqa: E731
                lines.append(f"| {s['scene']} | {label} | {q['hit_share']:.3f} | {cell('trace')} | {cell('occluded')} | "
                             f"{cell('features')} | {q['host_trace_kernel_ms']:.4f}, {q['host_occluded_kernel_ms']:.4f} |")
    text = "\n".join(lines) + "\n"
    with open(os.path.join(args.out, stem + ".md"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
