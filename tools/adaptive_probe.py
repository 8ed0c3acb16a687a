#!/usr/bin/env python3
"""tools/adaptive_probe.py — what rt_render_adaptive spends and what it buys.

For each configuration (bench.py's c4: final() 500x500, cap 1000; c3: random_motion()
800x400, cap 500) and each tolerance it reports

  * the samples spent (and the passes, converged and capped pixels),
  * the wall time of rt_render_adaptive against the fixed-spp rt_render_tile at the cap —
    both synchronous calls that end with the image in host memory, timed with a host clock,
    interleaved over --rounds rounds on the same device, medians; like a C caller, every
    call writes into the same host buffers,
  * the gamma-space RMS of both images against an independent fixed render at 4 x the cap
    with another seed.

Tolerance 0 is the overhead row: no pixel converges, every pixel gets the cap, the image is
the fixed render's bit for bit (asserted), and the extra time is the passes' launches and
selects.  --guard-radius adds rt_render_adaptive_guarded at each radius listed ("none" is
rt_render_adaptive itself).  Writes <out>/adaptive_probe.json and <out>/adaptive_probe.md.  Not run by any test.
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

CONFIGS = {"c4": ("final", 500, 500, 1000), "c3": ("random_motion", 800, 400, 500)}


def gamma_rms(a, b):
    ga, gb = np.sqrt(np.clip(a, 0.0, 1.0)), np.sqrt(np.clip(b, 0.0, 1.0))
    return float(np.sqrt(np.mean((ga - gb) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c3")
    ap.add_argument("--tolerances", default="0,0.05,0.1,0.2")
    ap.add_argument("--min-spp", type=int, default=32)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--guard-radius", default="none", help="comma-separated: none (rt_render_adaptive) or 0..8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the image side and the cap (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08"))
    args = ap.parse_args()
    radii = [None if r == "none" else int(r) for r in args.guard_radius.split(",")]
    tols = [(float(t), r) for t in args.tolerances.split(",") for r in radii]   # a variant: (tolerance, radius)
    os.makedirs(args.out, exist_ok=True)
    rows = []
    for cfg in args.configs.split(","):
        scene_name, nx, ny, cap = CONFIGS[cfg]
        nx, ny, cap = max(8, int(nx * args.scale)), max(8, int(ny * args.scale)), max(args.min_spp, int(cap * args.scale))
        cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene_name]
        scene = rtnw.Scene.builtin(scene_name)
        cam = rtnw.Camera.preset(cam_name, nx, ny)
        p = rtnw.RenderParams(nx, ny, cap, max_depth=depth, background=bg, seed=args.seed)
        pref = rtnw.RenderParams(nx, ny, 4 * cap, max_depth=depth, background=bg, seed=args.seed + 1)
        ref = scene.render_tile(cam, pref, 0, 0, nx, ny)

        L = rtnw.lib()
        buf_img = np.zeros((ny, nx, 3), np.float32)
        buf_spp = np.zeros((ny, nx), np.int32)
        buf_mom = np.zeros((ny, nx, 2), np.float32)

        def fixed():
            st = rtnw.RtStats()
            t0 = time.perf_counter()
            rc = L.rt_render_tile(scene.handle, ctypes.byref(cam.desc), ctypes.byref(p), 0, 0, nx, ny, buf_img.ctypes.data,
                                  ctypes.byref(st))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.rt_last_error()
            return ms, buf_img.copy(), st.as_dict()

        def adaptive(variant):
            tol, radius = variant
            ap_ = rtnw.RtAdaptiveParams(min_spp=args.min_spp, step_spp=args.step_spp, tolerance=tol, floor=args.floor)
            st = rtnw.RtAdaptiveStats()
            t0 = time.perf_counter()
            if radius is None:
                rc = L.rt_render_adaptive(scene.handle, ctypes.byref(cam.desc), ctypes.byref(p), ctypes.byref(ap_), 0, 0, nx,
                                          ny, buf_img.ctypes.data, buf_spp.ctypes.data, buf_mom.ctypes.data, ctypes.byref(st))
            else:
                rc = L.rt_render_adaptive_guarded(scene.handle, ctypes.byref(cam.desc), ctypes.byref(p), ctypes.byref(ap_),
                                                  radius, 0, 0, nx, ny, buf_img.ctypes.data, buf_spp.ctypes.data,
                                                  buf_mom.ctypes.data, ctypes.byref(st))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, L.rt_last_error()
            return ms, buf_img.copy(), buf_spp.copy(), st.as_dict()

        fixed()                                   # warm-up: code objects, buffers
        for tol in tols:
            adaptive(tol)
        t_fixed, t_adapt = [], {tol: [] for tol in tols}
        last = {}
        for _ in range(args.rounds):              # interleaved: drift hits every variant alike
            ms, img_f, st_f = fixed()
            t_fixed.append(ms)
            for tol in tols:
                ms, img, spp, st = adaptive(tol)
                t_adapt[tol].append(ms)
                last[tol] = (img, spp, st)
        fixed_ms = statistics.median(t_fixed)
        rms_fixed = gamma_rms(img_f, ref)
        print(f"{cfg}: {scene_name}() {nx}x{ny}, cap {cap}: fixed rt_render_tile {fixed_ms:.2f} ms wall "
              f"(min {min(t_fixed):.2f}, max {max(t_fixed):.2f}; kernel {st_f['kernel_ms']:.2f} ms), "
              f"gamma RMS vs {4 * cap} spp {rms_fixed:.5f}", flush=True)
        for variant in tols:
            tol, radius = variant
            img, spp, st = last[variant]
            if tol <= 0:
                assert np.array_equal(img.view(np.uint32), img_f.view(np.uint32)), "tolerance 0 is not the fixed render"
            ms = statistics.median(t_adapt[variant])
            row = {"guard_radius": radius, "select_ms_per_pass": st["select_ms"] / st["passes"], "config": cfg, "scene": scene_name, "nx": nx, "ny": ny, "cap": cap, "min_spp": args.min_spp,
                   "step_spp": args.step_spp, "floor": args.floor, "tolerance": tol, "rounds": args.rounds,
                   "samples": st["samples"], "samples_share": st["samples"] / (nx * ny * cap), "passes": st["passes"],
                   "pixels_converged": st["pixels_converged"], "pixels_capped": st["pixels_capped"],
                   "adaptive_ms": ms, "adaptive_ms_min": min(t_adapt[variant]), "adaptive_ms_max": max(t_adapt[variant]),
                   "fixed_ms": fixed_ms, "fixed_ms_min": min(t_fixed), "fixed_ms_max": max(t_fixed),
                   "kernel_ms": st["kernel_ms"], "resolve_ms": st["resolve_ms"], "select_ms": st["select_ms"],
                   "fixed_kernel_ms": st_f["kernel_ms"], "fixed_resolve_ms": st_f["resolve_ms"],
                   "rms_adaptive": gamma_rms(img, ref), "rms_fixed": rms_fixed,
                   "spp_mean": float(spp.mean()), "spp_median": float(np.median(spp))}
            rows.append(row)
            print(json.dumps(row), flush=True)
        scene.close()

    with open(os.path.join(args.out, "adaptive_probe.json"), "w") as f:
        json.dump({"tool": "tools/adaptive_probe.py", "args": vars(args), "rows": rows}, f, indent=1)
    with open(os.path.join(args.out, "adaptive_probe.md"), "w") as f:
        f.write("| config | tolerance | guard | samples (share of cap) | passes | converged / capped pixels | adaptive ms | "
                "fixed ms | kernel / resolve / select ms | gamma RMS adaptive | gamma RMS fixed |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['config']} {r['scene']} {r['nx']}x{r['ny']} cap {r['cap']} | {r['tolerance']:g} | "
                    f"{'none' if r['guard_radius'] is None else r['guard_radius']} | {r['samples']:.0f} ({r['samples_share']:.3f}) | {r['passes']:.0f} | "
                    f"{r['pixels_converged']:.0f} / {r['pixels_capped']:.0f} | {r['adaptive_ms']:.2f} | "
                    f"{r['fixed_ms']:.2f} | {r['kernel_ms']:.2f} / {r['resolve_ms']:.2f} / {r['select_ms']:.2f} | "
                    f"{r['rms_adaptive']:.5f} | {r['rms_fixed']:.5f} |\n")
    print(open(os.path.join(args.out, "adaptive_probe.md")).read())


if __name__ == "__main__":
    main()
