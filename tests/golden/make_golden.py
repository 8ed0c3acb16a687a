"""tests/golden/make_golden.py — regenerates the golden fixtures from the REFERENCE.

Runs oracle/_ref/ref_render (the reference compiled from /root/reference by
oracle/Makefile) in this container and records its outputs as data:

  golden.json        PPM MD5s (canonical drand48 runs, the reference's own RNG),
                     scene-dump SHA-256s, Perlin table hash, drand48 / counter-stream
                     known answers, and the SURVEY §8c MD5s it re-measures;
  ref_<cfg>.npy      small float framebuffers from counter-RNG reference runs
                     (mean radiance after `col /= float(ns)`, rows top-down);
  rays_hits_<scene>.npy, rays_radiance_<scene>.npy
                     512 caller-supplied rays each (tests/free_rays.py's families in the scene's
                     box) with what the reference's own world->hit and color() answered
                     (ref_harness.cpp's ray mode); hashes in golden.json.

Usage (container only; the reference never travels to the GPU box):
    make -C oracle && python tests/golden/make_golden.py          (everything)
    make -C oracle && python tests/golden/make_golden.py rays     (the ray fixtures alone)
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as O  # noqa: E402

# canonical (reference RNG) PPM goldens: (scene, nx, ny, ns)
CANONICAL = [
    ("final", 40, 40, 4), ("final", 100, 100, 10), ("random_scene", 200, 100, 10), ("cornell_box", 40, 40, 8),
    ("cornell_smoke", 32, 32, 4), ("random_motion", 40, 20, 4), ("simple_light", 40, 20, 4),
    ("two_spheres", 20, 20, 4), ("test", 20, 20, 4), ("earth", 40, 40, 8),
    ("edge_empty", 20, 10, 2), ("edge_single", 40, 20, 4), ("edge_degenerate", 40, 20, 8),
    ("edge_chains", 40, 20, 8),
]
# counter-RNG reference framebuffers: (name, scene, nx, ny, ns, seed)
COUNTER = [
    ("c1_random", "random_scene", 40, 20, 4, 1), ("c2_cornell", "cornell_box", 24, 24, 8, 2),
    ("c3_motion", "random_motion", 40, 20, 4, 3), ("c4_final", "final", 24, 24, 8, 4),
    ("smoke", "cornell_smoke", 24, 24, 8, 5), ("simple_light", "simple_light", 32, 16, 4, 6),
    ("earth", "earth", 32, 32, 8, 7),
    ("edge_empty", "edge_empty", 16, 8, 2, 12), ("edge_single", "edge_single", 32, 16, 8, 13),
    ("edge_degenerate", "edge_degenerate", 40, 20, 8, 14), ("edge_chains", "edge_chains", 40, 20, 8, 15),
]


# caller-supplied rays (tests/free_rays.py): per scene one fixture of 512 rt_ray records with the
# reference's own world->hit answers, and one of 512 rt_path_ray records with its color()
RAY_HITS = ["cornell_box", "random_motion", "simple_light", "earth"]            # media-free
RAY_RADIANCE = RAY_HITS + ["cornell_smoke", "edge_chains"]
RAY_SEED = 23
HIT_FIXTURE = np.dtype([("ray", O.RAY_DTYPE), ("ref", np.float32, O.REF_HIT_FIELDS)])
RADIANCE_FIXTURE = np.dtype([("ray", O.PATH_RAY_DTYPE), ("ref", np.float32, 3)])


def fixture_rays(scene):
    """The 512 rays of a built-in scene's fixtures: every family of tests/free_rays.py in the
    scene's box, family 1's hits answered by the oracle's built-in twin."""
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "peter-shirley-ray-tracing-the-next-week_amd")]
    import free_rays as R
    import rtnw
    from test_gpu_trace import bounds_of
    desc = rtnw.SceneDesc.builtin(scene, earth_png=O.EARTH_PNG)
    lo, hi = R.BUILTIN_BOX[scene]
    fam = R.all_families(desc, (lo, hi, 0.0, 1.0), RAY_SEED, lambda r: O.trace_rays(scene, r), bounds_of)
    return R.fixture_rays(fam), R


def ray_fixtures(g, work):
    g["ray_hits"], g["ray_radiance"] = {}, {}
    for scene in RAY_RADIANCE:
        rays, R = fixture_rays(scene)
        depth, bg, _ = O.RenderSpec(scene=scene).resolved()
        if scene in RAY_HITS:
            fx = np.zeros(len(rays), HIT_FIXTURE)
            fx["ray"], fx["ref"] = rays, O.ref_trace_rays(scene, rays, work)
            np.save(os.path.join(HERE, f"rays_hits_{scene}.npy"), fx)
            g["ray_hits"][scene] = dict(n=len(fx), hit_share=float(fx["ref"][:, 0].mean()),
                                        sha256=hashlib.sha256(fx.tobytes()).hexdigest())
        rec = R.path_records(rays, RAY_SEED)
        fx = np.zeros(len(rec), RADIANCE_FIXTURE)
        fx["ray"] = rec
        fx["ref"] = O.ref_radiance_rays(scene, rec, work, max_depth=depth, background=bg, seed=RAY_SEED)
        np.save(os.path.join(HERE, f"rays_radiance_{scene}.npy"), fx)
        g["ray_radiance"][scene] = dict(n=len(fx), max_depth=depth, background=bg, seed=RAY_SEED,
                                        lit_share=float((fx["ref"] > 0).any(axis=1).mean()),
                                        sha256=hashlib.sha256(fx.tobytes()).hexdigest())


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref/ref_render missing: run `make -C oracle` in the container that has /root/reference")
    work = tempfile.mkdtemp()
    if sys.argv[1:] == ["rays"]:   # the ray fixtures alone, added to the golden.json that is there
        with open(os.path.join(HERE, "golden.json")) as f:
            g = json.load(f)
        ray_fixtures(g, work)
        with open(os.path.join(HERE, "golden.json"), "w") as f:
            json.dump(g, f, indent=1, sort_keys=True)
        return
    g = {"generator": "tests/golden/make_golden.py", "reference_binary": "oracle/_ref/ref_render (clang++ -O2)"}
    g["canonical_ppm_md5"] = {}
    for sc, nx, ny, ns in CANONICAL:
        _, ppm, _ = O.ref_render(O.RenderSpec(scene=sc, nx=nx, ny=ny, ns=ns), work)
        g["canonical_ppm_md5"][f"{sc}_{nx}x{ny}x{ns}"] = hashlib.md5(ppm).hexdigest()
    g["scene_dump_sha256"] = {sc: hashlib.sha256(O.ref_dump(sc, work).encode()).hexdigest() for sc in O.SCENES}
    g["counter_fb"] = {}
    for name, sc, nx, ny, ns, seed in COUNTER:
        mean, _, _ = O.ref_render(O.RenderSpec(scene=sc, nx=nx, ny=ny, ns=ns, rng="counter", seed=seed), work)
        np.save(os.path.join(HERE, f"ref_{name}.npy"), mean)
        g["counter_fb"][name] = dict(scene=sc, nx=nx, ny=ny, ns=ns, seed=seed,
                                     sha256=hashlib.sha256(mean.tobytes()).hexdigest())
    # Perlin tables of the reference's static initialisers
    perlin = os.path.join(work, "perlin.bin")
    import subprocess
    subprocess.run([O.REF_BIN, "--scene", "two_spheres", "--nx", "1", "--ny", "1", "--ns", "1", "--perlin", perlin],
                   check=True, capture_output=True)
    g["perlin_sha256"] = hashlib.sha256(open(perlin, "rb").read()).hexdigest()
    # glibc drand48 from an unseeded state (the first values; SURVEY §8c: first = 3.9e-14)
    g["drand48_first"] = [float(x) for x in O.drand48_stream(0, 8)]
    g["counter_draws_seed7_px5_s3"] = [float(x) for x in O.counter_draws(7, 5, 3, 6)]
    g["medium_draw_seed7_px5_s3_b2_k1_of2"] = float(O.medium_draw(7, 5, 3, 2, 1, 2))
    g["survey_clang_md5"] = {"final_40x40x4": "9e7ff7c4c3b8f54d2d59bde695c06e4f",
                             "final_100x100x10": "593c5e4075645c45dc3760d885c21e3b"}
    ray_fixtures(g, work)
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(g, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "golden.json"))


if __name__ == "__main__":
    main()
