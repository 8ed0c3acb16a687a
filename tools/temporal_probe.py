#!/usr/bin/env python3
"""tools/temporal_probe.py — what the reprojected frame history buys and costs (rt_temporal;
DESIGN.md §7h).

1. Error over a camera move.  For random_scene and final() at 500 x 500 the camera takes --frames
   small steps; every frame is --spp fresh samples per pixel (sample_offset advanced by --spp) with
   its moments and first-hit guides.  Per frame the gamma RMS (square root of the clipped image,
   RMS over the pixels, mean of the channels) against a --ref-spp render of that same frame with
   another seed, of four images:

     raw            the frame
     denoised       rt_denoise of it (DENOISE_DEFAULTS, variance pre-filter on, its moments)
     accumulated    rt_temporal of it and the previous call's output
     acc+denoised   rt_denoise of that, rt_temporal's len as the spp map, its moments

   with cos_normal and sigma_depth at TEMPORAL_DEFAULTS and max_history swept over
   --max-history; the share of pixels that found a history and the mean len are reported along.

2. Cost.  The kernel's HIP-event time on 500 x 500 (median of --reps host-form calls after a
   warm-up; the event pair brackets the kernel alone) for a first frame, equal cameras and a
   reprojected frame, next to the bytes a call must move at the least — every input value read
   once, every output written once — and the GB/s that makes.

Writes <out>/temporal_probe.json and <out>/temporal_probe.md.  Not run by any test.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "peter-shirley-ray-tracing-the-next-week_amd"))
import rtnw  # noqa: E402

NX = NY = 500
# (scene, lookfrom of frame 0, lookfrom's step per frame, lookat, vfov, aperture): the presets of
# rtnw.CAMERA_PRESETS, moved sideways by a few pixels a frame
MOVES = {
    "random_scene": ((13.0, 2.0, 3.0), (0.0, 0.012, 0.05), (0.0, 0.0, 0.0), 20.0, 0.1),
    "final": ((228.0, 278.0, -800.0), (4.0, 0.5, 0.0), (278.0, 278.0, 0.0), 40.0, 0.0),
}


def gamma_rms(a, b):
    ga, gb = np.sqrt(np.clip(a, 0.0, 1.0)), np.sqrt(np.clip(b, 0.0, 1.0))
    return float(np.sqrt(np.mean((ga - gb) ** 2, axis=(0, 1))).mean())


def camera(scene, k):
    lf, step, lookat, vfov, aperture = MOVES[scene]
    pos = tuple(a + k * s for a, s in zip(lf, step))
    return rtnw.Camera(pos, lookat, (0, 1, 0), vfov, float(np.float32(NX) / np.float32(NY)), aperture, 10.0, 0.0, 1.0)


def run_scene(scene, args):
    _, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    sc = rtnw.Scene.builtin(scene)
    dn = dict(rtnw.DENOISE_DEFAULTS, variance_filter=1)
    hist = {h: None for h in args.max_history}
    prev_cam, rows = None, []
    for k in range(args.frames):
        cam = camera(scene, k)
        p = rtnw.RenderParams(NX, NY, args.spp, max_depth=depth, background=bg, seed=args.seed, chunk=1,
                              sample_offset=k * args.spp)
        color, mom = sc.render_tile_moments(cam, p, 0, 0, NX, NY)
        f = sc.render_features(cam, p, 0, 0, NX, NY)
        pr = rtnw.RenderParams(NX, NY, args.ref_spp, max_depth=depth, background=bg, seed=args.seed + 977)
        ref = sc.render_tile(cam, pr, 0, 0, NX, NY)
        row = dict(frame=k, raw=gamma_rms(color, ref),
                   denoised=gamma_rms(rtnw.denoise(color, f, mom, args.spp, **dn), ref), sweep={})
        for h in args.max_history:
            c, m, ln = rtnw.temporal(color, f, mom, args.spp, cam, hist[h], prev_cam, max_history=h)
            row["sweep"][str(h)] = dict(accumulated=gamma_rms(c, ref),
                                        acc_denoised=gamma_rms(rtnw.denoise(c, f, m, ln, **dn), ref),
                                        with_history=float((ln > args.spp).mean()), mean_len=float(ln.mean()))
            hist[h] = dict(color=c, moments=m, len=ln, features=f)
        prev_cam = cam
        rows.append(row)
        print(f"{scene} frame {k}: raw {row['raw']:.4f} denoised {row['denoised']:.4f} " +
              " ".join(f"[{h}: {v['accumulated']:.4f} {v['acc_denoised']:.4f} {v['with_history']:.2f}]"
                       for h, v in row["sweep"].items()), flush=True)
    # cost, on this scene's last two frames
    last = hist[args.max_history[-1]]
    before = camera(scene, args.frames - 2)
    times = {}
    for name, h, pc in (("first", None, None), ("equal", last, cam), ("reprojected", last, before)):
        ms = [rtnw.temporal(color, f, mom, args.spp, cam, h, pc, timing=True)[3] for _ in range(args.reps + 3)][3:]
        times[name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
    sc.close()
    return dict(scene=scene, frames=rows, kernel_ms=times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="temporal_probe_out")
    ap.add_argument("--scenes", nargs="+", default=list(MOVES))
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=512)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-history", type=int, nargs="+", default=[4, 8, 16, 32, 64, 128])
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    res = dict(nx=NX, ny=NY, frames=args.frames, spp=args.spp, ref_spp=args.ref_spp, max_history=args.max_history,
               settings={k: rtnw.TEMPORAL_DEFAULTS[k] for k in ("cos_normal", "sigma_depth")},
               scenes=[run_scene(s, args) for s in args.scenes])
    # the least a call moves per pixel: the frame (colour 12, guides 32, moments 8), the history
    # (colour 12, guides 32, moments 8, len 4) and the output (colour 12, moments 8, len 4)
    npix = NX * NY
    res["bytes"] = dict(first=npix * (12 + 8 + 12 + 8 + 4), equal=npix * (12 + 8 + 12 + 8 + 4 + 12 + 8 + 4),
                        reprojected=npix * (52 + 56 + 24))
    with open(os.path.join(args.out, "temporal_probe.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    md = [f"# tools/temporal_probe.py: {NX}x{NY}, {args.frames} frames of {args.spp} spp, gamma RMS against {args.ref_spp} spp "
          f"of the same frame with another seed; cos_normal {res['settings']['cos_normal']}, sigma_depth "
          f"{res['settings']['sigma_depth']}", ""]
    for s in res["scenes"]:
        hs = [str(h) for h in args.max_history]
        md += [f"## {s['scene']}", "", "accumulated / accumulated then denoised, per max_history", "",
               "| frame | raw | denoised | " + " | ".join(hs) + " | with history | mean len (" + hs[-1] + ") |",
               "|---|---|---|" + "---|" * (len(hs) + 2)]
        for r in s["frames"]:
            md.append(f"| {r['frame']} | {r['raw']:.4f} | {r['denoised']:.4f} | " +
                      " | ".join(f"{r['sweep'][h]['accumulated']:.4f} / {r['sweep'][h]['acc_denoised']:.4f}" for h in hs) +
                      f" | {r['sweep'][hs[-1]]['with_history']:.3f} | {r['sweep'][hs[-1]]['mean_len']:.1f} |")
        tail = s["frames"][len(s["frames"]) // 2:]
        mean = lambda g: sum(g(r) for r in tail) / len(tail)
        md.append(f"| mean of the last {len(tail)} | {mean(lambda r: r['raw']):.4f} | {mean(lambda r: r['denoised']):.4f} | " +
                  " | ".join(f"{mean(lambda r: r['sweep'][h]['accumulated']):.4f} / "
                             f"{mean(lambda r: r['sweep'][h]['acc_denoised']):.4f}" for h in hs) + " | | |")
        md += ["", "| call | kernel ms (median, min-max) | MB moved at the least | GB/s |", "|---|---|---|---|"]
        for name, t in s["kernel_ms"].items():
            b = res["bytes"][name]
            md.append(f"| {name} | {t['median_ms']:.4f} ({t['min_ms']:.4f}-{t['max_ms']:.4f}) | {b / 1e6:.1f} | "
                      f"{b / 1e9 / (t['median_ms'] / 1e3):.0f} |")
        md.append("")
    with open(os.path.join(args.out, "temporal_probe.md"), "w") as fh:
        fh.write("\n".join(md))
    print("\n".join(md))


if __name__ == "__main__":
    main()
