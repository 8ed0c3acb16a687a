"""The oracle's descriptor entry point (oracle_render_desc, oracle_first_hits_desc) pinned on the
CPU, and the generated cases of tests/gen_scenes.py checked before any GPU sees them.

  * on the built-in scenes (edge_chains included) the descriptor path (the host API's flattened descriptor,
    the preset camera handed over as a camera record) gives the image of the path the reference
    goldens pin (oracle.render of the oracle's own builders), bit for bit, in the kernel's
    statement and in the right-fold counter mode;
  * its first-hit mode agrees with the numpy restatement of tests/test_features_spec.py;
  * every generated case is a valid descriptor, its oracle image does not depend on the thread
    count or on rendering a crop, and it is not vacuous: without its target the image differs;
  * a medium without a boundary primitive is rejected by rt_scene_create.
"""
import ctypes

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
import test_features_spec as FS
from test_gpu_parity import CASES as PARITY_CASES

RT_ERR_INVALID, RT_ERR_HIP, RT_ERR_UNSUPPORTED = -1, -2, -4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def case_spec(c, **kw):
    kw.setdefault("chunk", c.spp)
    kw.setdefault("threads", 8)
    return O.desc_spec(c.nx, c.ny, c.spp, max_depth=c.max_depth, background=c.background, seed=c.seed, **kw)


# ------------------------------------------------------------------ the built-in scenes
@pytest.mark.parametrize("forward", [True, False], ids=["kernel", "right_fold"])
@pytest.mark.parametrize("scene,nx,ny,ns,chunk,seed", PARITY_CASES)
def test_descriptor_path_equals_builtin_path(scene, nx, ny, ns, chunk, seed, forward):
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    desc = rtnw.SceneDesc.builtin(scene, earth_png=O.EARTH_PNG)
    cam = rtnw.Camera.preset(cam_name, nx, ny)
    own = O.render(O.RenderSpec(scene=scene, nx=nx, ny=ny, ns=ns, rng="counter", seed=seed, media_after=True,
                                forward=forward, chunk=chunk, threads=8))[0]
    got = O.render_desc(desc, cam, O.desc_spec(nx, ny, ns, max_depth=depth, background="sky" if bg else "black",
                                               seed=seed, chunk=chunk, forward=forward, threads=8))[0]
    assert np.array_equal(bits(own), bits(got))


def test_descriptor_path_equals_builtin_path_in_list_order():
    """Media at their `order` places: the reference's own evaluation order (media inline, right
    fold) on the scenes that have media."""
    for scene, nx, ny, ns in (("cornell_smoke", 16, 16, 4), ("final", 16, 16, 4), ("edge_degenerate", 20, 10, 8)):
        cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
        own = O.render(O.RenderSpec(scene=scene, nx=nx, ny=ny, ns=ns, rng="counter", seed=3, threads=8))[0]
        got = O.render_desc(rtnw.SceneDesc.builtin(scene), rtnw.Camera.preset(cam_name, nx, ny),
                            O.desc_spec(nx, ny, ns, max_depth=depth, background="sky" if bg else "black", seed=3,
                                        forward=False, media_after=False, threads=8))[0]
        assert np.array_equal(bits(own), bits(got)), scene


def test_canonical_rng_is_refused():
    desc, cam = rtnw.SceneDesc.builtin("edge_single"), rtnw.Camera.preset("random", 4, 4)
    with pytest.raises(ValueError):
        O.render_desc(desc, cam, O.RenderSpec(scene="", nx=4, ny=4, ns=1, max_depth=5, background="sky"))


@pytest.mark.parametrize("scene", ["edge_single", "random_scene"])
def test_first_hit_mode_agrees_with_the_numpy_restatement(scene):
    """oracle_first_hits_desc against test_features_spec.first_hits (float64) on the samples
    that restatement decides, within its own TOL_NORMAL, TOL_DEPTH and MAX_UNDECIDED."""
    nx, ny, K, seed = FS.NX, FS.NY, FS.OFFSETS, FS.SEED
    draws = FS.jitter_draws(nx, ny, K, seed)
    desc, cam = rtnw.SceneDesc.builtin(scene), FS.pinhole_camera(scene, nx, ny)
    r64, _, keep = FS.compared(desc, cam, nx, ny, draws)
    assert 1.0 - keep.mean() <= FS.MAX_UNDECIDED
    fh = O.first_hits_desc(desc, cam, O.desc_spec(nx, ny, K, max_depth=50, background="sky", seed=seed))
    hit, prim = np.moveaxis(fh["hit"], -1, 0), np.moveaxis(fh["prim"], -1, 0)       # [K, ny, nx]
    depth, normal = np.moveaxis(fh["depth"], -1, 0), np.moveaxis(fh["normal"], 2, 0)
    assert np.array_equal(hit[keep], r64["hit"][keep])
    h = keep & r64["hit"]
    assert h.sum() > 100
    assert np.array_equal(prim[h], r64["prim"][h])
    assert np.abs(normal[h] - r64["normal"][h]).max() <= FS.TOL_NORMAL
    assert np.abs(depth[h] / r64["depth"][h] - 1).max() <= FS.TOL_DEPTH
    assert (depth[~hit] == 0).all() and (normal[~hit] == 0).all() and (fh["albedo"][~fh["hit"]] == 1).all()


# ------------------------------------------------------------------ the generated cases
@pytest.fixture(scope="module")
def images():
    """Every case's oracle image in the kernel's statement, rendered once."""
    out = {}
    for c in G.CASES:
        desc, cam = G.build(c)
        out[c.name] = O.render_desc(desc, cam, case_spec(c))[0]
    return out


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_generated_case_is_a_valid_descriptor(case):
    """Validation comes before the device check, so without a GPU a valid descriptor gets as
    far as RT_ERR_HIP (with one, the scene is created)."""
    desc, _ = G.build(case)
    h = ctypes.c_void_p()
    rc = rtnw.lib().rt_scene_create(desc.ptr, 0, ctypes.byref(h))
    msg = rtnw.lib().rt_last_error().decode()
    if rc == rtnw.RT_OK:
        rtnw.lib().rt_scene_destroy(h)
    elif rtnw.device_count() == 0:
        assert rc == RT_ERR_HIP, (rc, msg)
    else:
        pytest.fail(f"rt_scene_create: {rc} {msg}")


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_generated_oracle_image_is_independent_of_threads_and_crops(case, images):
    desc, cam = G.build(case)
    full = images[case.name]
    assert np.isfinite(full).all() and (full >= 0).all()
    one = O.render_desc(desc, cam, case_spec(case, threads=1))[0]
    assert np.array_equal(bits(one), bits(full))
    x0, y0, w, h = case.nx // 3, case.ny // 4, case.nx // 2, case.ny // 2
    crop = O.render_desc(desc, cam, case_spec(case, rect=(x0, y0, w, h)))[0]
    assert np.array_equal(bits(crop), bits(full[y0:y0 + h, x0:x0 + w]))


# Share of pixels whose oracle image differs when the case's target is removed (primitives and
# media dropped, textures replaced by grey), measured with this file's specs:
VACUITY_SHARES = """
scan64_mixed 0.276  scan65_mixed 0.276  scan64_spheres 0.107  scan64_own_chains 0.388  scan_five_kinds 0.195
prescan1 0.508  prescan8 0.695  prescan9 0.714
media8_scan 0.268  media9_scan 0.247  media12_scan 0.328  media9_bvh 0.281  media12_bvh 0.349
boundaries_scan 0.289  boundaries_bvh 0.307
cell_two_dense 0.299  cell_two_equal 0.276  cell_near4 0.224  cell_near5 0.229  cell_near_inst_moving 0.216
cell_dup_outside 0.268  cell_not_dense 0.315
ball_one_medium 0.682  ball_dense_first 0.840  ball_dense_second 0.838  ball_in_fog_on_ground 1.000
ball_full_cell 0.682  ball_thin 0.689  ball_negative_radius 0.678  ball_solid 0.678  ball_three_media 0.843
ball_noise_medium 0.844  ball_with_instance 0.837  ball_camera_inside 1.000
cloud1732 0.398  cloud1736 0.398  quad4095 0.250  quad4096 0.250  quad4095_cell_prescan 0.539
cloud1800_cell_prescan 0.609  progression200 0.148
chains_short 0.302  chains_long 0.336  image_rects 0.263  textures_by_kind 0.375
"""


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_generated_case_is_not_vacuous(case, images):
    """The case's target is in view: the oracle image without it differs in at least one pixel.
    Measured shares of differing pixels per case: VACUITY_SHARES above (0.107 to 1.000)."""
    b = case.builder()
    assert b.t_prims or b.t_media or b.t_textures, "the case names no target"
    plain = O.render_desc(b.desc(plain=True), case.camera(), case_spec(case))[0]
    share = float(np.mean(np.any(bits(plain) != bits(images[case.name]), axis=-1)))
    print(f"{case.name}: {share:.3f} of the pixels differ without the target")
    assert share > 0


def test_each_medium_from_the_ninth_on_is_visible_alone():
    """media9 / media12: dropping any single medium of index >= 8 (those media_hit reads from
    global memory, past the RT_LDS_MEDIA = 8 of the LDS copy) changes the image."""
    for name in ("media9_scan", "media12_scan", "media9_bvh", "media12_bvh"):
        c = G.BY_NAME[name]
        b = c.builder()
        full = O.render_desc(b.desc(), c.camera(), case_spec(c))[0]
        for m in range(8, len(b.media)):
            b.t_prims, b.t_media, b.t_textures = set(), {m}, set()
            without = O.render_desc(b.desc(plain=True), c.camera(), case_spec(c))[0]
            assert not np.array_equal(bits(without), bits(full)), (name, m)


def test_case_table_covers_both_sides_of_each_limit():
    """The structure the table's comments promise, counted from the descriptors."""
    n = {c.name: G.build(c)[0].contents for c in G.CASES}
    assert n["scan64_mixed"].nprims == 64 and n["scan65_mixed"].nprims == 65
    assert n["scan64_spheres"].nprims == 64 and n["scan64_own_chains"].ninstances == 64
    kinds = {n["scan_five_kinds"].prims[i].kind for i in range(n["scan_five_kinds"].nprims)}
    assert kinds == {0, 1, 2, 3, 4} and len({n["scan_five_kinds"].prims[i].instance for i in range(20)}) == 1
    assert [n[k].nmedia for k in ("media8_scan", "media9_scan", "media12_scan", "media9_bvh", "media12_bvh")] == [8, 9, 12, 9, 12]
    assert all(n[k].nprims <= 64 for k in ("media8_scan", "media9_scan", "media12_scan", "boundaries_scan"))
    assert all(n[k].nprims > 64 for k in n if k.startswith(("cell_", "prescan", "cloud", "quad")) or k.endswith("_bvh"))
    assert n["quad4095"].nprims == 4095 and n["quad4096"].nprims == 4096 and n["quad4095_cell_prescan"].nprims == 4095
    assert n["chains_short"].ninstances == 39
    assert max(n["chains_long"].instances[i].nops for i in range(n["chains_long"].ninstances)) == 6


def test_cross_group_ties_of_scan64_own_chains_are_in_view():
    """The last ten primitives are ties() with each member under a chain index of its own (equal
    ops): of the duplicate sphere and moving sphere the EARLIER is the first hit somewhere and
    the later never (sphere.h:33 needs t < t_max); each of the six coplanar rects is a first hit
    somewhere (aarect.h:50 accepts t == t_max, so the later wins where two overlap)."""
    c = G.BY_NAME["scan64_own_chains"]
    desc, cam = G.build(c)
    d = desc.contents
    assert d.nprims == 64 and len({d.prims[i].instance for i in range(64)}) == 64
    for a, b in ((54, 55), (56, 57)):
        assert list(d.prims[a].p) == list(d.prims[b].p) and d.prims[a].material != d.prims[b].material
        ia, ib = d.instances[d.prims[a].instance], d.instances[d.prims[b].instance]
        assert d.prims[a].instance != d.prims[b].instance and bytes(ia) == bytes(ib)
    seen = set(np.unique(O.first_hits_desc(desc, cam, case_spec(c))["prim"]).tolist())
    assert {54, 56, 58, 59, 60, 61, 62, 63} <= seen and not {55, 57} & seen, sorted(seen)


# ------------------------------------------------------------------ the medium cell, by scene_lower.cpp's rule
def prim_box(d, pr):
    """World box of a primitive over the shutter span [0, 1] (bvh.cpp prim_bounds without its
    outward padding, which is far below the margins the cases leave)."""
    p = list(pr.p)
    if pr.kind == G.SPHERE:
        lo, hi = np.array(p[0:3]) - abs(p[3]), np.array(p[0:3]) + abs(p[3])
    elif pr.kind == G.MSPHERE:
        c0, c1, r = np.array(p[0:3]), np.array(p[3:6]), abs(p[8])
        span = p[7] - p[6]
        ends = [c0 + ((t - p[6]) / span) * (c1 - c0) for t in (0.0, 1.0)] if span else [c0]
        lo, hi = np.min(ends, axis=0) - r, np.max(ends, axis=0) + r
    else:
        ax = {G.XY: (0, 1, 2), G.XZ: (0, 2, 1), G.YZ: (1, 2, 0)}[pr.kind]
        lo, hi = np.zeros(3), np.zeros(3)
        lo[ax[0]], hi[ax[0]], lo[ax[1]], hi[ax[1]], lo[ax[2]], hi[ax[2]] = p[0], p[1], p[2], p[3], p[4], p[4]
    if pr.instance >= 0:   # the box's corners through the chain, innermost (last) op first
        pts = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], float)
        inst = d.instances[pr.instance]
        for k in range(inst.nops - 1, -1, -1):
            op = list(inst.ops[k])
            if int(op[0]) == G.OP_T:
                pts = pts + np.array(op[1:4])
            elif int(op[0]) == G.OP_R:   # hitable.h:137-142: object to world
                s, c = op[1], op[2]
                pts = np.stack([c * pts[:, 0] + s * pts[:, 2], pts[:, 1], -s * pts[:, 0] + c * pts[:, 2]], 1)
        lo, hi = pts.min(0), pts.max(0)
    return lo, hi


def cell_choice(d):
    """scene_lower.cpp's medium-cell choice restated: (medium index or None, its near primitives) and
    the number of deep-first balls.  A candidate is a medium bounded by one un-instanced sphere
    (c, R); near = the primitives whose boxes come within R + R / 64 + 1e-3 |c|max of c; the
    cell goes to the first candidate of strictly greatest density with 1..RT_CELL_MAX = 4 near
    primitives; a ball is deep when 1 / density < R / 2."""
    best, chosen, near_of, deep = -1.0, None, [], 0
    boxes = [prim_box(d, d.prims[q]) for q in range(d.nprims)]
    for i in range(d.nmedia):
        m = d.media[i]
        bp = d.boundary_prims[m.boundary_first]
        if m.boundary_count != 1 or bp.kind != G.SPHERE or bp.instance >= 0:
            continue
        c, R = np.array(list(bp.p)[0:3]), abs(bp.p[3])
        if m.density > 0 and np.float32(1.0) / np.float32(m.density) < np.float32(0.5) * np.float32(R):
            deep += 1
        if not m.density > best:
            continue
        reach = R + R / 64 + 1e-3 * np.abs(c).max()
        near = [q for q, (lo, hi) in enumerate(boxes)
                if not (np.maximum(np.maximum(lo - c, c - hi), 0.0) ** 2).sum() > reach * reach]
        if 1 <= len(near) <= 4:
            best, chosen, near_of = m.density, i, near
    return chosen, near_of, deep


@pytest.mark.parametrize("name,medium,nnear,deep", [
    ("cell_two_dense", 1, 1, 2), ("cell_two_equal", 0, 1, 2),          # the denser; of equals the first
    ("cell_near4", 0, 4, 1), ("cell_near5", None, 0, 1),               # RT_CELL_MAX primitives taken, one more declined
    ("cell_near_inst_moving", 0, 4, 1), ("cell_dup_outside", 0, 4, 1),
    ("cell_not_dense", 1, 1, 1),                                        # 1 / 2 >= 0.45: only the second ball is deep
    ("quad4095_cell_prescan", 0, 1, 1), ("cloud1800_cell_prescan", 0, 1, 1),
    ("boundaries_bvh", None, 0, 0),                                     # no boundary is one plain sphere
    # the ball_* cases: the cell is the dense ball's (medium 1 where the second medium is listed first), with
    # the shell as its one near primitive, the ground where there is no shell, RT_CELL_MAX in full_cell
    ("ball_one_medium", 0, 1, 1), ("ball_dense_first", 0, 1, 1), ("ball_dense_second", 1, 1, 1),
    ("ball_in_fog_on_ground", 0, 1, 2),                                 # (the scene-wide fog counts as deep: 12.5 < 15)
    ("ball_full_cell", 0, 4, 1), ("ball_thin", 0, 1, 0), ("ball_negative_radius", 0, 1, 1), ("ball_solid", 0, 1, 1),
    ("ball_three_media", 0, 1, 1), ("ball_noise_medium", 0, 1, 1), ("ball_with_instance", 0, 1, 1),
    ("ball_camera_inside", 0, 4, 1)])
def test_medium_cell_choice_of_the_cases(name, medium, nnear, deep):
    """RTNW_CELL=0 in tests/test_gpu_generated.py proves something only where the cell is taken,
    and no rt_stats field shows that: the choice is recomputed here from each descriptor by
    scene_lower.cpp's rule, so the cases' intent (4 near primitives taken, 5 declined, ...) is asserted."""
    d = G.build(G.BY_NAME[name])[0].contents
    got_medium, near, got_deep = cell_choice(d)
    print(f"{name}: cell medium {got_medium}, near primitives {near}, deep balls {got_deep}")
    assert (got_medium, len(near), got_deep) == (medium, nnear, deep)
    if name == "cell_near_inst_moving":
        assert {d.prims[q].kind for q in near} == {G.SPHERE, G.MSPHERE, G.XY} and sum(d.prims[q].instance >= 0 for q in near) == 2
    if name.startswith("ball_"):
        bp = d.boundary_prims[d.media[got_medium].boundary_first]
        assert d.media[got_medium].density == np.float32(G.BALL_DENSITY[name[5:]]) and abs(bp.p[3]) == G.BALL_R
        assert d.nprims > 64 and d.ninstances == (1 if name == "ball_with_instance" else 0)
        kinds = sorted(d.prims[q].kind for q in near)
        if name in ("ball_full_cell", "ball_camera_inside"):   # the shell, a metal sphere, a moving sphere whose centres differ by more than its radius, a rect
            assert kinds == [G.SPHERE, G.SPHERE, G.MSPHERE, G.XZ]
            ms = [d.prims[q] for q in near if d.prims[q].kind == G.MSPHERE][0]
            assert np.linalg.norm(np.subtract(list(ms.p)[3:6], list(ms.p)[0:3])) > ms.p[8] > 0
        else:
            assert kinds == [G.XZ if name == "ball_in_fog_on_ground" else G.SPHERE]


def test_ball_cases_list_both_kinds():
    assert sorted(c.name for c in G.CASES if c.name.startswith("ball_")) == sorted("ball_" + v for v in G.BALL_QUALIFY + G.BALL_DECLINE)
    c = G.BY_NAME["ball_camera_inside"]   # its camera is inside the ball, the others' outside
    assert np.linalg.norm(np.subtract(c.lookfrom, G.ball_centre("camera_inside"))) < 0.8 * G.BALL_R
    assert all(np.linalg.norm(np.subtract(k.lookfrom, G.ball_centre(k.name[5:]))) > 2 * G.BALL_R
               for k in G.CASES if k.name.startswith("ball_") and k is not c)


def test_in_fog_on_ground_has_segments_the_cell_cannot_decide():
    """ball_in_fog_on_ground exists for the `best_t < tsafe` rule of the fused in-ball step: a
    segment that starts inside the ball and whose closest cell primitive (the ground, the only
    one) lies beyond the ball's exit, with a sphere outside the cell or a fog scatter before it.
    A float64 ray cast over the descriptor: origins uniform in the ball, directions uniform in the
    unit ball (what an isotropic scatter leaves behind: material.h:147), the fog's free path
    drawn as constant_medium.h:36 draws it.  At least 1 % of those segments must be such."""
    c = G.BY_NAME["ball_in_fog_on_ground"]
    d = G.build(c)[0].contents
    medium, near, _ = cell_choice(d)
    bp, fog = d.boundary_prims[d.media[medium].boundary_first], d.media[1 - medium]
    cc, R = np.array(list(bp.p)[0:3], float), abs(bp.p[3])
    assert near == [0] and d.prims[0].kind == G.XZ and fog.density < 0.1   # (the ground is primitive 0)
    rng = np.random.default_rng(7)
    n = 20000
    v = rng.normal(size=(n, 3))
    o = cc + R * rng.uniform(size=(n, 1)) ** (1 / 3) * v / np.linalg.norm(v, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3))
    dirs = rng.uniform(size=(n, 1)) ** (1 / 3) * w / np.linalg.norm(w, axis=1, keepdims=True)

    def sphere_t(centre, rad):   # the smallest root above t_min, inf where none
        oc = o - centre
        a, hb, k = (dirs * dirs).sum(1), (oc * dirs).sum(1), (oc * oc).sum(1) - rad * rad
        disc = hb * hb - a * k
        s = np.sqrt(np.maximum(disc, 0))
        t0, t1 = (-hb - s) / a, (-hb + s) / a
        t = np.where(t0 > 1e-3, t0, np.where(t1 > 1e-3, t1, np.inf))
        return np.where(disc > 0, t, np.inf)
    t_exit = sphere_t(cc, R)
    g = list(d.prims[0].p)
    tg = (g[4] - o[:, 1]) / dirs[:, 1]
    x, z = o[:, 0] + tg * dirs[:, 0], o[:, 2] + tg * dirs[:, 2]
    tg = np.where((tg > 1e-3) & (x > g[0]) & (x < g[1]) & (z > g[2]) & (z < g[3]), tg, np.inf)
    others = np.full(n, np.inf)
    for q in range(1, d.nprims):
        assert d.prims[q].kind == G.SPHERE
        others = np.minimum(others, sphere_t(np.array(list(d.prims[q].p)[0:3], float), abs(d.prims[q].p[3])))
    fog_t = -(1.0 / fog.density) * np.log(rng.uniform(size=n)) / np.linalg.norm(dirs, axis=1)   # the camera and the ball are inside the fog
    undecided = np.isfinite(tg) & (tg > t_exit) & (np.minimum(others, fog_t) < tg)
    print(f"ball_in_fog_on_ground: ground beyond the exit {np.mean(np.isfinite(tg) & (tg > t_exit)):.3f}, with a sphere before "
          f"it {np.mean(undecided & (others < tg)):.3f}, a fog scatter before it {np.mean(undecided & (fog_t < tg)):.3f}, "
          f"either {undecided.mean():.3f}")
    assert undecided.mean() >= 0.01


def test_every_case_with_a_medium_cell_compares_it():
    """Whichever BVH case the rule gives a cell (the cell_* cases by design, others by the way)
    lists RTNW_CELL among its knobs, so test_gpu_generated compares the image without it."""
    for c in G.CASES:
        d = G.build(c)[0].contents
        if d.nprims > 64 and d.nmedia and cell_choice(d)[0] is not None:
            assert "RTNW_CELL" in c.knobs, c.name


# ------------------------------------------------------------------ empty medium boundary
@pytest.mark.parametrize("nboundary", [0, 1])
def test_medium_without_boundary_is_rejected(nboundary):
    """boundary_count == 0 (with nboundary == 0 the empty range passes the range check): the
    device would read the medium's first boundary record, one past the array."""
    b = G.Builder(np.random.default_rng(1))
    b.add(b.sphere((0, 0, 0), 1, b.lambert()))
    b.medium(b.sphere((0, 0, 0), 2, b.glass()), 0.5, b.const(1, 1, 1))
    b.medium(b.sphere((0, 0, 0), 3, b.glass()), 0.1, b.const(1, 1, 1))
    b.media[1]["count"] = 0
    if nboundary == 0:
        b.media, b.boundary = [dict(b.media[1], first=0)], []
    desc = b.desc()
    assert desc.contents.nboundary == nboundary and desc.contents.media[desc.contents.nmedia - 1].boundary_count == 0
    h = ctypes.c_void_p()
    rc = rtnw.lib().rt_scene_create(desc.ptr, 0, ctypes.byref(h))
    msg = rtnw.lib().rt_last_error().decode()
    assert rc == RT_ERR_UNSUPPORTED, (rc, msg)
    assert f"medium {0 if nboundary == 0 else 1}" in msg and "boundary" in msg, msg
    assert not h.value
