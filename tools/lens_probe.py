#!/usr/bin/env python3
"""tools/lens_probe.py — what a lens render costs (rt_render_lens).

1. The panorama.  The --pano-width x --pano-width / 2 equirectangular view of final() from
   --pano-eye at --pano-spp samples, with moments and guides, timed with device events on one
   stream, in one session, the forms taking turns (median of --rounds rounds after a warm-up
   round, min - max beside it):

     generate   rt_lens_rays_dev: every record and its trace ray (96 B written per sample)
     query      rt_radiance_rays_dev on those records (48 B read, 16 B written per sample)
     trace      rt_trace_rays_dev on the trace rays (48 B read, 48 B written per sample)
     render     rt_render_lens_dev: generate, query, trace and resolve per batch, at the default
                batch size, and in one batch (RTNW_LENS_BATCH raised to the whole job)
     resolve    not a call of its own: the one-batch render minus the three above (derived)
     image      rt_render_lens_dev without moments and guides

   Beside it the same picture made by hand, as tools/radiance_probe.py makes it: the records
   written in numpy, rt_radiance_rays' host form, the mean taken on the host; its kernel time, its
   wall time, and the bytes each way moves over PCIe.

2. The perspective lens render of final() at 500 x 500 x --spp against rt_render_tiles(chunk = 1)
   of the same frame, taking turns; the two images are compared bit for bit first.

--kernels runs part 1's render three times and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`, whose per-kernel times are the direct split.

Writes <out>/lens_probe.json and <out>/lens_probe.md.  Not run by any test.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rtnw  # noqa: E402


def span(ms, n=None):
    med = statistics.median(ms)
    out = dict(ms=med, ms_min=min(ms), ms_max=max(ms))
    if n:
        out["msamples_per_s"] = n / med / 1e3
    return out


def event_ms(fn, stream):
    """Device time of fn()'s enqueues on the stream, between two events."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def take_turns(forms, rounds, stream):
    ms = {k: [] for k in forms}
    for r in range(rounds + 1):           # round 0 warms up
        for k, fn in forms.items():
            t = event_ms(fn, stream)
            if r:
                ms[k].append(t)
    return ms


def pano_setup(args):
    w, h, spp = args.pano_width, args.pano_width // 2, args.pano_spp
    eye = tuple(args.pano_eye)
    cam = rtnw.Camera(eye, (eye[0], eye[1], eye[2] + 1.0), (0, 1, 0), 40.0, w / h, 0.0, 10.0, 0.0, 1.0)
    _, bg, depth = rtnw.SCENE_DEFAULTS["final"]
    p = rtnw.RenderParams(w, h, spp, max_depth=depth, background=bg, chunk=1, seed=args.seed)
    return w, h, spp, cam, p, rtnw.lens_params(rtnw.RT_LENS_EQUIRECT)


def panorama(args):
    import torch
    import radiance_probe
    scene = rtnw.Scene.builtin("final")
    w, h, spp, cam, p, lens = pano_setup(args)
    n = w * h * spp
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    d_rays = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_tr = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_rad = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_hit = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    d_img = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    d_mom = torch.zeros(h * w * 2, dtype=torch.float32, device=dev)
    d_gd = torch.zeros(h * w * 8, dtype=torch.float32, device=dev)

    def render(batch):
        def go():
            if batch:
                os.environ["RTNW_LENS_BATCH"] = str(batch)
            else:
                os.environ.pop("RTNW_LENS_BATCH", None)
            scene.render_lens_dev(cam, p, lens, 0, 0, w, h, d_img.data_ptr(), d_mom.data_ptr(), d_gd.data_ptr(), sp)
        return go

    def image():
        os.environ.pop("RTNW_LENS_BATCH", None)
        scene.render_lens_dev(cam, p, lens, 0, 0, w, h, d_img.data_ptr(), 0, 0, sp)

    whole = 1 << 24
    assert n <= whole, "the one-batch form needs the job within RTNW_LENS_BATCH's largest value"
    forms = dict(
        generate=lambda: rtnw.lens_rays_dev(cam, p, lens, 0, 0, w, h, d_rays.data_ptr(), d_tr.data_ptr(), sp),
        query=lambda: scene.radiance_rays_dev(p, d_rays.data_ptr(), n, d_rad.data_ptr(), sp),
        trace=lambda: scene.trace_rays_dev(d_tr.data_ptr(), n, d_hit.data_ptr(), sp),
        render=render(0), render_one_batch=render(whole), image=image)
    ms = take_turns(forms, args.rounds, stream)
    os.environ.pop("RTNW_LENS_BATCH", None)
    out = {k: span(v, n) for k, v in ms.items()}
    parts = out["generate"]["ms"] + out["query"]["ms"] + out["trace"]["ms"]
    out["resolve_derived_ms"] = out["render_one_batch"]["ms"] - parts
    out["generate_plus_resolve_over_query"] = (out["generate"]["ms"] + out["resolve_derived_ms"]) / out["query"]["ms"]
    # the device render against the queries on its own records, at the timed size
    torch.cuda.synchronize()
    rad = d_rad.cpu().numpy().view(rtnw.RADIANCE_DTYPE)["rgb"].reshape(spp, h * w, 3)
    acc = np.zeros((h * w, 3), np.float32)
    for s in range(spp):
        acc = acc + rad[s]
    out["render_equals_its_records_reduced"] = bool(np.array_equal((acc * np.float32(1.0 / spp)).view(np.uint32),
                                                                  d_img.cpu().numpy().reshape(h * w, 3).view(np.uint32)))
    # the host form, and the picture made by hand
    t0 = time.perf_counter()
    img, mom, gd, host_ms = scene.render_lens(cam, p, lens, 0, 0, w, h, moments=True, guides=True, timing=True)
    host_wall = (time.perf_counter() - t0) * 1e3
    np.save(os.path.join(args.out, "lens_panorama_final.npy"), img)
    out["host_form"] = dict(kernel_ms=host_ms, wall_ms=host_wall, pcie_bytes_up=0, pcie_bytes_down=h * w * 13 * 4,
                            mean=float(img.mean()), lit_share=float((img.sum(-1) > 0).mean()),
                            coverage=float(gd[..., 3].mean()))
    scene.close()
    hand_args = argparse.Namespace(out=args.out, pano_width=w, pano_spp=spp, pano_eye=args.pano_eye, seed=args.seed)
    t0 = time.perf_counter()
    hand = radiance_probe.panorama(hand_args)
    out["by_hand"] = dict(kernel_ms=hand["kernel_ms"], wall_ms=(time.perf_counter() - t0) * 1e3, pcie_bytes_up=n * 48,
                          pcie_bytes_down=n * 16, mean=hand["mean"], lit_share=hand["lit_share"])
    out.update(width=w, height=h, spp=spp, samples=n, eye=list(map(float, args.pano_eye)),
               record_bytes_per_sample=dict(generate_written=96, query_read=48, query_written=16, trace_read=48,
                                            trace_written=48, resolve_read=64))
    return out


def perspective(args):
    import torch
    scene = rtnw.Scene.builtin("final")
    nx = ny = 500
    spp = args.spp
    _, bg, depth = rtnw.SCENE_DEFAULTS["final"]
    cam = rtnw.Camera.preset("cornell", nx, ny)
    p = rtnw.RenderParams(nx, ny, spp, max_depth=depth, background=bg, chunk=1, seed=args.seed)
    lens = rtnw.lens_params(rtnw.RT_LENS_PERSPECTIVE)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    d_a = torch.zeros(ny * nx * 3, dtype=torch.float32, device=dev)
    d_b = torch.zeros(ny * nx * 3, dtype=torch.float32, device=dev)
    forms = dict(lens=lambda: scene.render_lens_dev(cam, p, lens, 0, 0, nx, ny, d_a.data_ptr(), 0, 0, sp),
                 tiles=lambda: scene.render_tiles(cam, p, [(0, 0, nx, ny)], d_b.data_ptr(), sp, stats=False))
    ms = take_turns(forms, args.rounds, stream)
    torch.cuda.synchronize()
    n = nx * ny * spp
    out = dict(nx=nx, ny=ny, spp=spp, samples=n, lens=span(ms["lens"], n), tiles=span(ms["tiles"], n),
               identical=bool(torch.equal(d_a.view(torch.int32), d_b.view(torch.int32))))
    out["lens_over_tiles"] = out["lens"]["ms"] / out["tiles"]["ms"]
    scene.close()
    return out


def kernels_only(args):
    import torch
    scene = rtnw.Scene.builtin("final")
    w, h, spp, cam, p, lens = pano_setup(args)
    dev = torch.device("cuda", 0)
    d_img = torch.zeros(h * w * 3, dtype=torch.float32, device=dev)
    d_mom = torch.zeros(h * w * 2, dtype=torch.float32, device=dev)
    d_gd = torch.zeros(h * w * 8, dtype=torch.float32, device=dev)
    for _ in range(3):
        scene.render_lens_dev(cam, p, lens, 0, 0, w, h, d_img.data_ptr(), d_mom.data_ptr(), d_gd.data_ptr(), 0)
    torch.cuda.synchronize()
    scene.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="lens_probe_out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--pano-width", type=int, default=1024)
    ap.add_argument("--pano-spp", type=int, default=16)
    ap.add_argument("--pano-eye", type=float, nargs=3, default=(278.0, 278.0, 100.0))
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if rtnw.device_count() < 1:
        sys.exit("lens_probe: no GPU (there is no CPU path to time)")
    if args.kernels:
        return kernels_only(args)
    os.makedirs(args.out, exist_ok=True)
    res = dict(lib=os.path.basename(rtnw.LIB_PATH), version=rtnw.lib().rt_version().decode(), rounds=args.rounds,
               panorama=panorama(args), perspective=perspective(args))
    with open(os.path.join(args.out, "lens_probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    q, v = res["panorama"], res["perspective"]
    cell = lambda d: f"{d['ms']:.3f} ({d['ms_min']:.3f} - {d['ms_max']:.3f})"  # noqa: E731
    lines = [f"# lens_probe: device-event times on one stream, median of {args.rounds} rounds taking turns (min - max)", "",
             f"## equirect panorama of final(), {q['width']} x {q['height']} x {q['spp']} = {q['samples']} samples from {q['eye']}",
             "", "| form | ms | Msamples/s |", "|---|---|---|"]
    for k in ("generate", "query", "trace", "render", "render_one_batch", "image"):
        lines.append(f"| {k} | {cell(q[k])} | {q[k]['msamples_per_s']:.1f} |")
    lines += ["", f"resolve (derived: one-batch render minus generate, query and trace): {q['resolve_derived_ms']:.3f} ms; "
                  f"generate plus resolve over the query: {q['generate_plus_resolve_over_query']:.3f}; "
                  f"the render equals its records reduced: {q['render_equals_its_records_reduced']}", "",
              "| picture | kernel ms | wall ms | PCIe bytes up | PCIe bytes down | mean | lit share |", "|---|---|---|---|---|---|---|"]
    for k, name in (("host_form", "rt_render_lens (host form, moments and guides)"), ("by_hand", "by hand (radiance_probe.panorama)")):
        d = q[k]
        lines.append(f"| {name} | {d['kernel_ms']:.2f} | {d['wall_ms']:.0f} | {d['pcie_bytes_up']} | {d['pcie_bytes_down']} | "
                     f"{d['mean']:.4f} | {d['lit_share']:.3f} |")
    lines += ["", f"## perspective lens render of final(), {v['nx']} x {v['ny']} x {v['spp']}, against rt_render_tiles(chunk = 1)", "",
              "| form | ms | Msamples/s |", "|---|---|---|", f"| rt_render_lens_dev | {cell(v['lens'])} | {v['lens']['msamples_per_s']:.1f} |",
              f"| rt_render_tiles | {cell(v['tiles'])} | {v['tiles']['msamples_per_s']:.1f} |", "",
              f"lens over tiles: {v['lens_over_tiles']:.3f}; images identical bit for bit: {v['identical']}"]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(args.out, "lens_probe.md"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
