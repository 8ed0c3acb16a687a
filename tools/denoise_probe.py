#!/usr/bin/env python3
"""tools/denoise_probe.py — what the feature pass and the denoiser cost and what they buy.

For each configuration (bench.py's c4: final() 500x500, cap 1000; c3: random_motion() 800x400,
cap 500) it runs render -> features -> denoise twice, from the fixed render at the cap (with
moments, uniform count) and from rt_render_adaptive at DESIGN.md §7b's settings (min_spp 32,
step_spp 64, floor 0.01, tolerance 0.05; its moments and count map), and reports

  * the samples spent,
  * the ms of each stage: the synchronous host calls' wall times (render, features, denoise)
    as medians over --rounds interleaved rounds, and the denoiser's kernel time (HIP events),
  * the gamma-space RMS against an independent fixed render at 4 x the cap with another seed,
    before and after the filter.

--variance-filter 1 adds every row once more with rt_denoise_params.variance_filter on, and
--guard-radius R renders the adaptive input with rt_render_adaptive_guarded.
--sweep adds the grid over sigma_color, sigma_depth and iterations that chose the defaults
(rtnw.DENOISE_DEFAULTS): the gamma RMS of every setting on all four inputs.
--timing adds the denoiser's kernel ms for 1..5 iterations (the first figure holds the prepare
kernel) and the feature pass's wall ms on 500x500 and 1000x1000.

--firefly adds every row once more with the firefly clamp (rt_firefly, rtnw.FIREFLY_DEFAULTS)
ahead of the filter: the clamped pixels, the clamp's kernel ms and the gamma RMS of the clamped
image before and after the filter.  With --sweep it runs, in place of the
filter's grid, the grid over k and radius that chose those defaults, with --timing the clamp's
kernel ms by radius beside the à-trous iterations'.  --cap overrides the configurations' sample
caps (a low-count regime).

Writes <out>/denoise_probe.json and <out>/denoise_probe.md.  Not run by any test.
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def features_dev_ms(scene, cam, p, nx, ny, rounds):
    """Wall ms of rt_render_features_dev on the default stream, ended by a 4-byte copy back."""
    L = rtnw.lib()
    dev = ctypes.c_void_p()
    rtnw._check(L.rt_device_alloc(0, nx * ny * 32, ctypes.byref(dev)))
    word = np.zeros(1, np.float32)
    try:
        def run():
            scene.render_features_dev(cam, p, 0, 0, nx, ny, dev.value)
            rtnw._check(L.rt_copy_to_host(word.ctypes.data, dev, 4))
        run()
        return statistics.median(timed(run)[0] for _ in range(rounds))
    finally:
        L.rt_device_free(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c3")
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--min-spp", type=int, default=32)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--feature-spp", type=int, default=16)
    ap.add_argument("--variance-filter", type=int, default=0, choices=(0, 1), help="1: rows with the pre-filter too")
    ap.add_argument("--guard-radius", type=int, default=None, help="the adaptive input's guard radius (0..8)")
    ap.add_argument("--firefly", action="store_true", help="rows with the firefly clamp ahead of the filter too")
    ap.add_argument("--cap", type=int, default=None, help="overrides the configurations' sample caps")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the image side and the cap (rehearsals)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    rows, sweep, timing = [], [], []
    for cfg in args.configs.split(","):
        scene_name, nx, ny, cap = CONFIGS[cfg]
        nx, ny, cap = max(8, int(nx * args.scale)), max(8, int(ny * args.scale)), max(args.min_spp, int(cap * args.scale))
        if args.cap:
            cap = max(args.min_spp, args.cap)
        cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene_name]
        scene = rtnw.Scene.builtin(scene_name)
        cam = rtnw.Camera.preset(cam_name, nx, ny)
        p = rtnw.RenderParams(nx, ny, cap, max_depth=depth, background=bg, seed=args.seed, chunk=1)
        pf = rtnw.RenderParams(nx, ny, args.feature_spp, seed=args.seed)
        pref = rtnw.RenderParams(nx, ny, 4 * cap, max_depth=depth, background=bg, seed=args.seed + 1)
        ref = scene.render_tile(cam, pref, 0, 0, nx, ny)

        def fixed():
            color, mom = scene.render_tile_moments(cam, p, 0, 0, nx, ny)
            return color, mom, cap, float(nx * ny * cap)

        def adaptive():
            color, spp, mom, st = scene.render_adaptive(cam, p, 0, 0, nx, ny, min_spp=args.min_spp, step_spp=args.step_spp,
                                                        tolerance=args.tolerance, floor=args.floor,
                                                        guard_radius=args.guard_radius)
            return color, mom, spp, st["samples"]

        def feats():
            return scene.render_features(cam, pf, 0, 0, nx, ny)

        renders = {"fixed": fixed, "adaptive": adaptive}
        for fn in (fixed, adaptive, feats):     # warm-up: code objects, buffers
            fn()
        t = {k: [] for k in ("fixed", "adaptive", "features", "denoise_fixed", "denoise_adaptive")}
        kms = {"fixed": [], "adaptive": []}
        last = {}
        for _ in range(args.rounds):            # interleaved: drift hits every stage alike
            ms, f = timed(feats)
            t["features"].append(ms)
            for name, fn in renders.items():
                ms, (color, mom, spp, samples) = timed(fn)
                t[name].append(ms)
                ms, (out, k) = timed(lambda: rtnw.denoise(color, f, mom, spp, timing=True))
                t["denoise_" + name].append(ms)
                kms[name].append(k)
                last[name] = (color, mom, spp, samples, out)
        feat_ms = statistics.median(t["features"])
        for name in renders:
            color, mom, spp, samples, out = last[name]
            row = {"config": cfg, "scene": scene_name, "nx": nx, "ny": ny, "cap": cap, "input": name,
                   "tolerance": args.tolerance if name == "adaptive" else None, "feature_spp": args.feature_spp,
                   "samples": samples, "samples_share": samples / (nx * ny * cap), **rtnw.DENOISE_DEFAULTS,
                   "render_ms": statistics.median(t[name]), "features_ms": feat_ms,
                   "denoise_ms": statistics.median(t["denoise_" + name]), "denoise_kernel_ms": statistics.median(kms[name]),
                   "rms_raw": gamma_rms(color, ref), "rms_denoised": gamma_rms(out, ref), "variance_filter": 0,
                   "guard_radius": args.guard_radius if name == "adaptive" else None, "firefly": 0}
            row["total_raw_ms"] = row["render_ms"]
            row["total_denoised_ms"] = row["render_ms"] + row["features_ms"] + row["denoise_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.variance_filter:            # the same input through the pre-filter
                runs = [timed(lambda: rtnw.denoise(color, f, mom, spp, variance_filter=1, timing=True))
                        for _ in range(args.rounds + 1)][1:]
                row = dict(row, variance_filter=1, denoise_ms=statistics.median(ms for ms, _ in runs),
                           denoise_kernel_ms=statistics.median(k for _, (_, k) in runs),
                           rms_denoised=gamma_rms(runs[-1][1][0], ref))
                row["total_denoised_ms"] = row["render_ms"] + row["features_ms"] + row["denoise_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
        if args.firefly:                        # the same inputs through the clamp, then the filter
            for name in renders:
                color, mom, spp, samples, _ = last[name]
                runs = [rtnw.firefly(color, f, mom, want_ratio=True, timing=True) for _ in range(args.rounds + 2)][2:]
                cl, cmom, ratio, _ = runs[-1]
                base = next(r for r in rows if r["config"] == cfg and r["input"] == name and r["variance_filter"] == 0
                            and not r["firefly"])
                for vf in ((0, 1) if args.variance_filter else (0,)):
                    dn = [timed(lambda: rtnw.denoise(cl, f, cmom, spp, variance_filter=vf, timing=True))
                          for _ in range(args.rounds + 1)][1:]
                    row = dict(base, variance_filter=vf, firefly=1, **{"firefly_" + k: v for k, v in rtnw.FIREFLY_DEFAULTS.items()},
                               firefly_kernel_ms=statistics.median(r[3] for r in runs), clamped_pixels=int((ratio != 1).sum()),
                               rms_clamped=gamma_rms(cl, ref), denoise_ms=statistics.median(ms for ms, _ in dn),
                               denoise_kernel_ms=statistics.median(k for _, (_, k) in dn),
                               rms_denoised=gamma_rms(dn[-1][1][0], ref))
                    row["total_denoised_ms"] = row["render_ms"] + row["features_ms"] + row["denoise_ms"]
                    rows.append(row)
                    print(json.dumps(row), flush=True)
        if args.firefly and args.sweep:         # the grid that chose rtnw.FIREFLY_DEFAULTS
            for k in (2.0, 4.0, 8.0, 16.0):
                for radius in (1, 2):
                    r = {"config": cfg, "firefly_k": k, "firefly_radius": radius}
                    for name in renders:
                        color, mom, spp, _, _ = last[name]
                        cl, cmom, ratio = rtnw.firefly(color, f, mom, k=k, radius=radius, want_ratio=True)
                        r["clamped_" + name] = int((ratio != 1).sum())
                        r["rms_clamped_" + name] = gamma_rms(cl, ref)
                        for vf in (0, 1):
                            r[f"rms_vf{vf}_" + name] = gamma_rms(rtnw.denoise(cl, f, cmom, spp, variance_filter=vf), ref)
                    sweep.append(r)
                    print(json.dumps(r), flush=True)
            r = {"config": cfg, "firefly_k": None, "firefly_radius": None}   # the clamp off, for comparison
            for name in renders:
                color, mom, spp, _, _ = last[name]
                r["rms_clamped_" + name] = gamma_rms(color, ref)
                for vf in (0, 1):
                    r[f"rms_vf{vf}_" + name] = gamma_rms(rtnw.denoise(color, f, mom, spp, variance_filter=vf), ref)
            sweep.append(r)
            print(json.dumps(r), flush=True)
        elif args.sweep:
            for it in (3, 4, 5, 6):
                for sc in (1.0, 2.0, 4.0, 8.0, 16.0):
                    for sd in (0.25, 1.0, 4.0):
                        for dm in (1, 0):
                            if dm == 0 and (sc, sd) != (4.0, 1.0):
                                continue        # demodulation off: one setting per iteration count
                            r = {"config": cfg, "iterations": it, "sigma_color": sc, "sigma_depth": sd, "demodulate": dm}
                            for name in renders:
                                color, mom, spp, _, _ = last[name]
                                out = rtnw.denoise(color, f, mom, spp, iterations=it, demodulate=dm, sigma_color=sc,
                                                   sigma_depth=sd)
                                r["rms_" + name] = gamma_rms(out, ref)
                            sweep.append(r)
                            print(json.dumps(r), flush=True)
            # the guides' sample count: the defaults with features of 1, 4, 16, 64 spp
            for fs in (1, 4, 16, 64):
                ff = scene.render_features(cam, rtnw.RenderParams(nx, ny, fs, seed=args.seed), 0, 0, nx, ny)
                r = {"config": cfg, "feature_spp": fs}
                for name in renders:
                    color, mom, spp, _, _ = last[name]
                    r["rms_" + name] = gamma_rms(rtnw.denoise(color, ff, mom, spp), ref)
                sweep.append(r)
                print(json.dumps(r), flush=True)
        if args.timing and cfg == "c4":
            color, mom, spp, _, _ = last["fixed"]
            for rep in (1, 2):                  # 500 x 500, and the same data tiled to 1000 x 1000
                c2, m2 = np.tile(color, (rep, rep, 1)), np.tile(mom, (rep, rep, 1))
                f2 = {k: np.tile(v, (rep, rep, 1) if v.ndim == 3 else (rep, rep)) for k, v in f.items()}
                r = {"nx": nx * rep, "ny": ny * rep}
                for it in range(1, 6):
                    ks = [rtnw.denoise(c2, f2, m2, spp, iterations=it, timing=True)[1] for _ in range(7)]
                    r[f"kernel_ms_{it}_iterations"] = statistics.median(ks[2:])
                if args.firefly:                # the clamp's kernel by radius, on the same data
                    for radius in (1, 2, 3):
                        ks = [rtnw.firefly(c2, f2, m2, radius=radius, timing=True)[-1] for _ in range(9)]
                        r[f"firefly_kernel_ms_radius_{radius}"] = statistics.median(ks[2:])
                timing.append(r)
                print(json.dumps(r), flush=True)
            for rep in (1, 2):
                cam2 = rtnw.Camera.preset(cam_name, nx * rep, ny * rep)
                for fs in (1, 4, 16):
                    pf2 = rtnw.RenderParams(nx * rep, ny * rep, fs, seed=args.seed)
                    r = {"nx": nx * rep, "ny": ny * rep, "feature_spp": fs,
                         "features_dev_ms": features_dev_ms(scene, cam2, pf2, nx * rep, ny * rep, 5)}
                    timing.append(r)
                    print(json.dumps(r), flush=True)
        scene.close()

    with open(os.path.join(args.out, "denoise_probe.json"), "w") as f:
        json.dump({"tool": "tools/denoise_probe.py", "args": vars(args), "rows": rows, "sweep": sweep, "timing": timing},
                  f, indent=1)
    with open(os.path.join(args.out, "denoise_probe.md"), "w") as f:
        f.write("| config | input | firefly clamp (pixels clamped, kernel ms, gamma RMS clamped) | variance filter | samples (share of cap) | render ms | features ms | denoise ms (kernels) | total raw ms | "
                "total denoised ms | gamma RMS raw | gamma RMS denoised |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['config']} {r['scene']} {r['nx']}x{r['ny']} cap {r['cap']} | {r['input']}"
                    f"{'' if r['guard_radius'] is None else ' guard ' + str(r['guard_radius'])} | "
                    + (f"on ({r['clamped_pixels']}, {r['firefly_kernel_ms']:.4f}, {r['rms_clamped']:.5f})" if r["firefly"] else "off")
                    + f" | {r['variance_filter']} | "
                    f"{r['samples']:.0f} ({r['samples_share']:.3f}) | {r['render_ms']:.2f} | {r['features_ms']:.2f} | "
                    f"{r['denoise_ms']:.2f} ({r['denoise_kernel_ms']:.3f}) | {r['total_raw_ms']:.2f} | "
                    f"{r['total_denoised_ms']:.2f} | {r['rms_raw']:.5f} | {r['rms_denoised']:.5f} |\n")
    print(open(os.path.join(args.out, "denoise_probe.md")).read())


if __name__ == "__main__":
    main()
