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

--clamp measures rt_temporal_clamped over the same camera moves instead: per frame
the gamma RMS of the accumulated image for every max_history of --max-history, unclamped
(rt_temporal) and clamped at every radius of --radius and gamma of --gamma, each setting carrying
its own history, with the share of the pixels whose history the clamp moved; the unclamped
accumulation at max_history 16, the yardstick, once more on frames drawn with another seed
(--seed + 1), whose distance from the first run is the spread a difference must exceed to mean
anything; and the kernel's time for a reprojected frame, rt_temporal's and the clamped entry
point's at radius 1, 2 and 3.  Writes
<out>/temporal_clamp_probe.md and .json (the table's numbers; per frame only the unclamped and
the tightest box's series).

--cover measures rt_temporal_cover over the same camera moves at max_history 16:
plain (rt_temporal's rule), background only, and background and edges at every sigma_coverage of
--sigma-coverage, each without a clamp and with the --cover-clamp one (radius 1, gamma 0.5), each
setting carrying its own history: the gamma RMS of the accumulated image, the share of the pixels
per `source` value and the share of the histories the clamp moved; rt_temporal once more on frames
drawn with another seed, for the spread; and the kernel's time for a reprojected frame, rt_temporal's
and rt_temporal_clamped's own kernels beside the cover kernel's with nothing and with everything on.
Writes <out>/temporal_cover_probe.md and .json.
"""
import argparse
import json
import os
import re
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


def clamp_scene(scene, args):
    _, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    sc = rtnw.Scene.builtin(scene)
    settings = [(h, 0, 0.0) for h in args.max_history] + \
               [(h, r, g) for h in args.max_history for r in args.radius for g in args.gamma]
    hist = {s: None for s in settings}
    repeat_hist, prev_cam, rows = None, None, []
    for k in range(args.frames):
        cam = camera(scene, k)

        def frame(seed):
            p = rtnw.RenderParams(NX, NY, args.spp, max_depth=depth, background=bg, seed=seed, chunk=1,
                                  sample_offset=k * args.spp)
            return sc.render_tile_moments(cam, p, 0, 0, NX, NY) + (sc.render_features(cam, p, 0, 0, NX, NY),)
        color, mom, f = frame(args.seed)
        pr = rtnw.RenderParams(NX, NY, args.ref_spp, max_depth=depth, background=bg, seed=args.seed + 977)
        ref = sc.render_tile(cam, pr, 0, 0, NX, NY)
        row = dict(frame=k, raw=gamma_rms(color, ref), error={}, clipped={})
        for s in settings:
            h, r, g = s
            c, m, ln, clip = rtnw.temporal_clamped(color, f, mom, args.spp, cam, hist[s], prev_cam, max_history=h, radius=r,
                                                   gamma=g)
            row["error"][key(s)] = gamma_rms(c, ref)
            row["clipped"][key(s)] = float((clip != 0).sum() / max(1, (ln > args.spp).sum()))
            hist[s] = dict(color=c, moments=m, len=ln, features=f)
        # the yardstick once more, on other samples of the same frames
        color2, mom2, f2 = frame(args.seed + 1)
        c, m, ln = rtnw.temporal(color2, f2, mom2, args.spp, cam, repeat_hist, prev_cam, max_history=YARDSTICK)
        row["repeat"] = gamma_rms(c, ref)
        repeat_hist = dict(color=c, moments=m, len=ln, features=f2)
        prev_cam = cam
        rows.append(row)
        best = min(row["error"], key=row["error"].get)
        print(f"{scene} frame {k}: raw {row['raw']:.4f} " +
              " ".join(f"[{h} unclamped {row['error'][key((h, 0, 0.0))]:.4f}]" for h in args.max_history) +
              f" repeat {row['repeat']:.4f} best {best} {row['error'][best]:.4f}", flush=True)
    # cost, on this scene's last two frames: a reprojected call of rt_temporal itself, then of the clamped entry
    # point at every radius (with the mask, which its kernel writes)
    last = hist[(YARDSTICK, 0, 0.0)]
    before = camera(scene, args.frames - 2)
    times = {}
    for r in [0] + list(args.radius):
        call = (lambda: rtnw.temporal(color, f, mom, args.spp, cam, last, before, timing=True)[3]) if r == 0 else \
               (lambda: rtnw.temporal_clamped(color, f, mom, args.spp, cam, last, before, radius=r, gamma=1.0, timing=True)[4])
        ms = [call() for _ in range(args.reps + 3)][3:]
        times["rt_temporal" if r == 0 else f"radius {r}"] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
    sc.close()
    return dict(scene=scene, frames=rows, kernel_ms=times)


YARDSTICK = 16   # the unclamped max_history every setting is held against (TEMPORAL_DEFAULTS')


def key(s):
    h, r, g = s
    return f"{h} unclamped" if r == 0 else f"{h} r{r} g{g:g}"


def clamp_main(args):
    if YARDSTICK not in args.max_history:
        args.max_history = [YARDSTICK] + args.max_history
    res = dict(nx=NX, ny=NY, frames=args.frames, spp=args.spp, ref_spp=args.ref_spp, max_history=args.max_history,
               radius=args.radius, gamma=args.gamma,
               settings={k: rtnw.TEMPORAL_DEFAULTS[k] for k in ("cos_normal", "sigma_depth")},
               scenes=[clamp_scene(s, args) for s in args.scenes])
    clamp_report(res, args.out)


def clamp_report(res, out):
    """The table (.md) and its numbers (.json: per setting the mean over the second half of the
    frames, the last frame's error and the clipped share; per frame only the raw, the unclamped
    and the tightest box's series, which show the drift)."""
    os.makedirs(out, exist_ok=True)
    hs, rs, gs, nf = res["max_history"], res["radius"], res["gamma"], res["frames"]
    tail = range(nf // 2, nf)
    md = [f"# tools/temporal_probe.py --clamp: {NX}x{NY}, {nf} frames of {res['spp']} spp, gamma RMS of the accumulated "
          f"frame against {res['ref_spp']} spp of the same frame with another seed, mean over frames {tail[0]}-{tail[-1]} "
          f"(and the last frame's); cos_normal {res['settings']['cos_normal']}, sigma_depth {res['settings']['sigma_depth']}", ""]
    scenes = []
    for s in res["scenes"]:
        rows = s["frames"]
        mean = lambda get: sum(get(rows[k]) for k in tail) / len(tail)
        tail_mean = {n: mean(lambda r: r["error"][n]) for n in rows[0]["error"]}
        tail_clipped = {n: mean(lambda r: r["clipped"][n]) for n in rows[0]["clipped"]}
        repeat, yard = mean(lambda r: r["repeat"]), key((YARDSTICK, 0, 0.0))
        spread = abs(repeat - tail_mean[yard])
        per_frame = [abs(rows[k]["repeat"] - rows[k]["error"][yard]) for k in tail]   # the two runs, frame by frame
        best = min(tail_mean, key=tail_mean.get)
        md += [f"## {s['scene']}", "",
               f"raw {mean(lambda r: r['raw']):.4f}; unclamped max_history {YARDSTICK}: {tail_mean[yard]:.4f}, on "
               f"other samples {repeat:.4f} (the means differ by {spread:.6f}; frame by frame the two runs differ by "
               f"{sum(per_frame) / len(per_frame):.5f} in the mean and {max(per_frame):.5f} at the most); lowest: {best} "
               f"{tail_mean[best]:.4f}", "",
               "mean error (last frame's error; share of the pixels with history that the clamp moved)", "",
               "| max_history | unclamped | radius | " + " | ".join(f"gamma {g:g}" for g in gs) + " |",
               "|---|---|---|" + "---|" * len(gs)]
        for h in hs:
            for r in rs:
                u = key((h, 0, 0.0))
                md.append(f"| {h} | {tail_mean[u]:.4f} ({rows[-1]['error'][u]:.4f}) | {r} | " + " | ".join(
                    f"{tail_mean[n]:.4f} ({rows[-1]['error'][n]:.4f}; {tail_clipped[n]:.2f})"
                    for n in (key((h, r, g)) for g in gs)) + " |")
        md += ["", "| reprojected call | kernel ms (median, min-max) |", "|---|---|"]
        for name, t in s["kernel_ms"].items():
            md.append(f"| {name} | {t['median_ms']:.4f} ({t['min_ms']:.4f}-{t['max_ms']:.4f}) |")
        md.append("")
        shown = [key((h, 0, 0.0)) for h in hs] + [key((h, rs[0], gs[0])) for h in hs]
        series = {n: [round(r["error"][n], 5) for r in rows] for n in shown}
        series.update(raw=[round(r["raw"], 5) for r in rows], repeat=[round(r["repeat"], 5) for r in rows])
        scenes.append(dict(scene=s["scene"], yardstick=round(tail_mean[yard], 6), repeat=round(repeat, 6),
                           spread=round(spread, 6), per_frame_spread_mean=round(sum(per_frame) / len(per_frame), 6),
                           per_frame_spread_max=round(max(per_frame), 6), lowest=best,
                           kernel_ms={n: [round(t[k], 5) for k in ("median_ms", "min_ms", "max_ms")]
                                      for n, t in s["kernel_ms"].items()},
                           mean_last_clipped={n: [round(tail_mean[n], 5), round(rows[-1]["error"][n], 5),
                                                  round(tail_clipped[n], 3)] for n in tail_mean},
                           per_frame=series))
    small = dict({k: v for k, v in res.items() if k != "scenes"}, tail=[tail[0], tail[-1]], scenes=scenes)
    text = re.sub(r"\[[^\[\]{}]*\]", lambda m: re.sub(r"\s+", " ", m.group(0)), json.dumps(small, indent=1))   # a list a line
    with open(os.path.join(out, "temporal_clamp_probe.json"), "w") as fh:
        fh.write(text + "\n")
    with open(os.path.join(out, "temporal_clamp_probe.md"), "w") as fh:
        fh.write("\n".join(md))
    print("\n".join(md))


def cover_settings(args):
    """(background, edges, sigma_coverage, radius, gamma): plain, background only, background and
    edges at every --sigma-coverage; each without a clamp and with the --cover-clamp one."""
    classes = [(0, 0, 0.0), (1, 0, 0.0)] + [(1, 1, s) for s in args.sigma_coverage]
    return [c + k for k in ((0, 0.0), tuple(args.cover_clamp)) for c in classes]


def cover_key(s):
    b, e, sg, r, g = s
    name = "plain" if not b and not e else "background" if not e else f"background+edges s{sg:g}"
    return name + (f", r{r} g{g:g}" if r else "")


def cover_scene(scene, args):
    _, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    sc = rtnw.Scene.builtin(scene)
    settings = cover_settings(args)
    hist = {s: None for s in settings}
    repeat_hist, prev_cam, rows = None, None, []
    for k in range(args.frames):
        cam = camera(scene, k)

        def frame(seed):
            p = rtnw.RenderParams(NX, NY, args.spp, max_depth=depth, background=bg, seed=seed, chunk=1,
                                  sample_offset=k * args.spp)
            return sc.render_tile_moments(cam, p, 0, 0, NX, NY) + (sc.render_features(cam, p, 0, 0, NX, NY),)
        color, mom, f = frame(args.seed)
        pr = rtnw.RenderParams(NX, NY, args.ref_spp, max_depth=depth, background=bg, seed=args.seed + 977)
        ref = sc.render_tile(cam, pr, 0, 0, NX, NY)
        cov = np.asarray(f["coverage"], np.float32).reshape(NY, NX)
        row = dict(frame=k, raw=gamma_rms(color, ref), error={}, source={}, clipped={},
                   coverage=[float((cov == 0).mean()), float(((cov > 0) & (cov < 1)).mean()), float((cov == 1).mean())])
        for s in settings:
            b, e, sg, r, g = s
            c, m, ln, clip, src = rtnw.temporal_cover(color, f, mom, args.spp, cam, hist[s], prev_cam, max_history=YARDSTICK,
                                                      background=b, edges=e, sigma_coverage=sg, radius=r, gamma=g)
            row["error"][cover_key(s)] = gamma_rms(c, ref)
            row["source"][cover_key(s)] = {str(v): float((src == v).mean()) for v in (0, 1, 2, 5, 6)}
            row["clipped"][cover_key(s)] = float((clip != 0).sum() / max(1, (src != 0).sum()))
            hist[s] = dict(color=c, moments=m, len=ln, features=f)
        # the yardstick (rt_temporal itself) once more, on other samples of the same frames
        color2, mom2, f2 = frame(args.seed + 1)
        c, m, ln = rtnw.temporal(color2, f2, mom2, args.spp, cam, repeat_hist, prev_cam, max_history=YARDSTICK)
        row["repeat"] = gamma_rms(c, ref)
        repeat_hist = dict(color=c, moments=m, len=ln, features=f2)
        prev_cam = cam
        rows.append(row)
        print(f"{scene} frame {k}: raw {row['raw']:.4f} repeat {row['repeat']:.4f} " +
              " ".join(f"[{n}: {v:.4f}]" for n, v in row["error"].items()), flush=True)
    # cost, on this scene's last two frames: a reprojected call of rt_temporal's and rt_temporal_clamped's own kernels,
    # then of the cover kernel (mask and source written) with nothing on, and with everything on, at radius 0 and 1
    last = hist[settings[0]]
    before = camera(scene, args.frames - 2)
    r1, g1 = args.cover_clamp
    calls = {
        "rt_temporal": lambda: rtnw.temporal(color, f, mom, args.spp, cam, last, before, timing=True)[3],
        f"rt_temporal_clamped r{r1}": lambda: rtnw.temporal_clamped(color, f, mom, args.spp, cam, last, before, radius=r1, gamma=g1,
                                                                   timing=True)[4],
    }
    for name, (b, e) in (("plain", (0, 0)), ("background+edges", (1, 1))):
        for r in (0, r1):
            calls[f"rt_temporal_cover {name} r{r}"] = \
                lambda b=b, e=e, r=r: rtnw.temporal_cover(color, f, mom, args.spp, cam, last, before, background=b, edges=e,
                                                          sigma_coverage=0.25, radius=r, gamma=g1, timing=True)[5]
    times = {}
    for name, call in calls.items():
        ms = [call() for _ in range(args.reps + 3)][3:]
        times[name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
    sc.close()
    return dict(scene=scene, frames=rows, kernel_ms=times)


def cover_report(res, out):
    """The table (.md) and its numbers (.json: per setting the mean over the second half of the
    frames of the error, of the share of pixels per source value and of the clipped share; per
    frame the raw, the repeat and every setting's error)."""
    os.makedirs(out, exist_ok=True)
    nf = res["frames"]
    tail = range(nf // 2, nf)
    md = [f"# tools/temporal_probe.py --cover: {NX}x{NY}, {nf} frames of {res['spp']} spp, gamma RMS of the accumulated frame "
          f"against {res['ref_spp']} spp of the same frame with another seed, mean over frames {tail[0]}-{tail[-1]} (and the "
          f"last frame's); max_history {YARDSTICK}, cos_normal {res['settings']['cos_normal']}, sigma_depth "
          f"{res['settings']['sigma_depth']}; clamp: radius {res['cover_clamp'][0]:g}, gamma {res['cover_clamp'][1]:g}", ""]
    scenes = []
    for s in res["scenes"]:
        rows = s["frames"]
        mean = lambda get: sum(get(rows[k]) for k in tail) / len(tail)
        names = list(rows[0]["error"])
        err = {n: mean(lambda r: r["error"][n]) for n in names}
        src = {n: {v: mean(lambda r: r["source"][n][v]) for v in rows[0]["source"][n]} for n in names}
        clip = {n: mean(lambda r: r["clipped"][n]) for n in names}
        covg = [mean(lambda r: r["coverage"][i]) for i in range(3)]
        repeat = mean(lambda r: r["repeat"])
        per_frame = [abs(rows[k]["repeat"] - rows[k]["error"]["plain"]) for k in tail]
        md += [f"## {s['scene']}", "",
               f"raw {mean(lambda r: r['raw']):.4f}; plain (rt_temporal's rule): {err['plain']:.4f}, rt_temporal on other samples "
               f"{repeat:.4f} (frame by frame the two runs differ by {sum(per_frame) / len(per_frame):.5f} in the mean and "
               f"{max(per_frame):.5f} at the most); coverage 0 on {covg[0]:.3f} of the pixels, partial on {covg[1]:.3f}, 1 on "
               f"{covg[2]:.3f}; lowest: {min(err, key=err.get)} {err[min(err, key=err.get)]:.4f}", "",
               "| setting | error (last frame's) | against plain | source 0 | 1 | 2 | 5 | 6 | clipped |", "|---|---|---|---|---|---|---|---|---|"]
        for n in names:
            base = err["plain, " + n.split(", ", 1)[1]] if ", " in n else err["plain"]
            md.append(f"| {n} | {err[n]:.4f} ({rows[-1]['error'][n]:.4f}) | {100 * (err[n] / base - 1):+.1f} % | " +
                      " | ".join(f"{src[n][v]:.3f}" for v in ("0", "1", "2", "5", "6")) + f" | {clip[n]:.2f} |")
        md += ["", "| reprojected call | kernel ms (median, min-max) |", "|---|---|"]
        for name, t in s["kernel_ms"].items():
            md.append(f"| {name} | {t['median_ms']:.4f} ({t['min_ms']:.4f}-{t['max_ms']:.4f}) |")
        md.append("")
        scenes.append(dict(scene=s["scene"], repeat=round(repeat, 6), per_frame_spread_mean=round(sum(per_frame) / len(per_frame), 6),
                           per_frame_spread_max=round(max(per_frame), 6), coverage=[round(v, 4) for v in covg],
                           kernel_ms={n: [round(t[k], 5) for k in ("median_ms", "min_ms", "max_ms")]
                                      for n, t in s["kernel_ms"].items()},
                           mean_last_clipped={n: [round(err[n], 5), round(rows[-1]["error"][n], 5), round(clip[n], 3)] for n in names},
                           source={n: [round(src[n][v], 4) for v in ("0", "1", "2", "5", "6")] for n in names},
                           per_frame=dict({n: [round(r["error"][n], 5) for r in rows] for n in names},
                                          raw=[round(r["raw"], 5) for r in rows], repeat=[round(r["repeat"], 5) for r in rows])))
    small = dict({k: v for k, v in res.items() if k != "scenes"}, tail=[tail[0], tail[-1]], scenes=scenes)
    text = re.sub(r"\[[^\[\]{}]*\]", lambda m: re.sub(r"\s+", " ", m.group(0)), json.dumps(small, indent=1))   # a list a line
    with open(os.path.join(out, "temporal_cover_probe.json"), "w") as fh:
        fh.write(text + "\n")
    with open(os.path.join(out, "temporal_cover_probe.md"), "w") as fh:
        fh.write("\n".join(md))
    print("\n".join(md))


def cover_main(args):
    res = dict(nx=NX, ny=NY, frames=args.frames, spp=args.spp, ref_spp=args.ref_spp, max_history=YARDSTICK,
               sigma_coverage=args.sigma_coverage, cover_clamp=args.cover_clamp,
               settings={k: rtnw.TEMPORAL_DEFAULTS[k] for k in ("cos_normal", "sigma_depth")},
               scenes=[cover_scene(s, args) for s in args.scenes])
    cover_report(res, args.out)


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
    ap.add_argument("--clamp", action="store_true", help="measure rt_temporal_clamped instead (see above)")
    ap.add_argument("--radius", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--gamma", type=float, nargs="+", default=[0.5, 1.0, 1.5, 2.0, 3.0])
    ap.add_argument("--cover", action="store_true", help="measure rt_temporal_cover instead (see above)")
    ap.add_argument("--sigma-coverage", type=float, nargs="+", default=[0.125, 0.25, 0.5, 1.0])
    ap.add_argument("--cover-clamp", type=float, nargs=2, default=[1, 0.5], metavar=("RADIUS", "GAMMA"))
    args = ap.parse_args()
    args.cover_clamp = (int(args.cover_clamp[0]), float(args.cover_clamp[1]))
    if args.cover:
        return cover_main(args)
    if args.clamp:
        return clamp_main(args)
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
