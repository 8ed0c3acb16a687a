"""Ray families for the queries on caller-supplied rays (rt_trace_rays, rt_occluded,
rt_radiance_rays; tests/test_free_rays_spec.py on the CPU, tests/test_gpu_free_rays.py on the GPU):
rays that no pinhole or thin-lens camera makes.  A plain module like gen_scenes.py: numpy only,
fixed seeds, float32 throughout (float64 appears only where a point is carried through an
instance chain, and is rounded once).  Nothing here touches a GPU or the oracle: the two
families that start from the hits of another take those hits as an argument.

Given a scene's world box (lo, hi) and time span (t0, t1), each family is N = 1,536 rt_ray records:

  1 inside_out   origins uniform in the box grown by a margin, directions uniform on the sphere,
                 times uniform over the span; t_min 0.001, t_max +inf.
  2 continued    origin = o + t * d (float32) of family 1's hits, taken in turn (alternately from the
                 hits on spheres and on rects), so the ray starts on the surface it hit, at that
                 ray's time; a fresh uniform direction of length 1, 2, 4 or 8; t_min 0.001, 0 and
                 -0.5 dealt by index.
  3 grazing      rays aimed at a sphere's silhouette (centre + r * u with u normal to the
                 direction, the origin then moved by 0, +-1, +-4 ulps along u) and at points whose
                 coordinates are exactly a rect's a0 / a1 / b0 / b1; every other ray looks upwards,
                 so that one which passes its target may leave the scene.  The ray is made in the
                 primitive's own frame in float64, carried through the chain to the world there and
                 rounded once: both sides then see the same float32 ray, whatever it hits.
  4 bounded      family 1's first 1,024 rays with t_max dealt around the hit's own t (t, its two
                 neighbours, t / 2, 2 t, FLT_MAX: `bounds_of`, an argument); 256 rays from outside
                 towards the box with t_max below the distance to it; 256 rays from beyond the box
                 looking away with a negative t_min: hits behind the origin.
  5 scaled       family 1's first 768 rays with the direction times 2^-20, and again times 2^20
                 (t_min scaled the other way: the same segment of space).

path_records() deals the radiance queries' key fields over a family by index: pixel and sample
over the whole uint32 range with 0 and 2^32 - 1 among them, skip in {0, 1, 5, 6, 191, 192}.
hand_placed() puts origins inside every dielectric sphere, inside every medium's boundary and
on every light of a descriptor.

Out of scope, by the contract in rt_hip.h and stated here so that nothing is left out silently:
  * subnormal direction components (2^-20 keeps every component normal);
  * exactly axis-parallel rays on rects: no family makes a direction component of exactly 0
    (test_free_rays_spec asserts it wherever a scene has rects).
"""
import numpy as np

import rtnw

F = np.float32
N = 1536
FAMILIES = ("inside_out", "continued", "grazing", "bounded", "scaled")
T_MINS = (F(0.001), F(0.0), F(-0.5))
SKIPS = (0, 1, 5, 6, 191, 192)
SPHERE, MSPHERE = 0, 1
OP_T, OP_R = 1, 2

# the boxes the built-in scenes' fixtures are made in (tests/golden/make_golden.py): the part
# of each scene its objects stand in, not the 700-unit ground spheres' own extent
BUILTIN_BOX = {
    "cornell_box": ((0, 0, 0), (555, 555, 555)), "cornell_smoke": ((0, 0, 0), (555, 555, 555)),
    "earth": ((60, 50, 50), (490, 560, 490)), "random_motion": ((-11, 0, -11), (11, 2.5, 11)),
    "simple_light": ((-6, 0, -6), (6, 9, 6)), "edge_chains": ((-6, 0, -6), (6, 4.5, 6)),
}


# ------------------------------------------------------------------ descriptors
def prims_of(desc, boundary=False):
    c = desc.contents
    return [c.boundary_prims[i] for i in range(c.nboundary)] if boundary else [c.prims[i] for i in range(c.nprims)]


def chain_of(desc, prim):
    """The primitive's ops, ops[0] outermost: [(kind, a, b, c)]."""
    if prim.instance < 0:
        return []
    inst = desc.contents.instances[prim.instance]
    return [tuple(float(x) for x in inst.ops[k]) for k in range(inst.nops)]


def to_world(ops, p):
    """A point of the primitive's frame in the world (float64): the innermost op first."""
    p = np.array(p, np.float64)
    for kind, a, b, c in reversed(ops):
        if int(kind) == OP_T:
            p = p + (a, b, c)
        elif int(kind) == OP_R:               # hitable.h:141-144: sin a, cos b
            p = np.array([b * p[0] + a * p[2], p[1], -a * p[0] + b * p[2]])
    return p


def prim_corners(p):
    """The corners of a primitive's box in its own frame."""
    q = [float(x) for x in p.p]
    if p.kind == SPHERE:
        lo, hi = np.subtract(q[0:3], abs(q[3])), np.add(q[0:3], abs(q[3]))
    elif p.kind == MSPHERE:
        r = abs(q[8])
        lo, hi = np.minimum(q[0:3], q[3:6]) - r, np.maximum(q[0:3], q[3:6]) + r
    else:
        ia, ib, ik = {2: (0, 1, 2), 3: (0, 2, 1), 4: (1, 2, 0)}[p.kind]
        lo, hi = np.zeros(3), np.zeros(3)
        lo[ia], hi[ia], lo[ib], hi[ib], lo[ik], hi[ik] = q[0], q[1], q[2], q[3], q[4], q[4]
    return [np.where([i & 1, i & 2, i & 4], hi, lo) for i in range(8)]


def extent(desc):
    """(lo, hi, t0, t1) of a descriptor: the world box of its surface and boundary primitives."""
    pts = [to_world(chain_of(desc, p), c) for b in (False, True) for p in prims_of(desc, b) for c in prim_corners(p)]
    c = desc.contents
    return np.min(pts, axis=0).astype(F), np.max(pts, axis=0).astype(F), F(c.time0), F(c.time1)


# ------------------------------------------------------------------ draws
def unit(rng, n):
    """n directions uniform on the sphere, float64, no component within 1e-3 of zero."""
    out = np.zeros((0, 3))
    while len(out) < n:
        v = rng.normal(size=(2 * n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        out = np.concatenate([out, v[(np.abs(v) > 1e-3).all(axis=1)]])
    return out[:n]


def times(rng, n, t0, t1):
    return np.clip((F(t0) + rng.random(n).astype(F) * (F(t1) - F(t0))).astype(F), F(t0), F(t1))


def grown(lo, hi, margin=0.15):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    m = np.maximum(margin * (hi - lo), 0.05 * (hi - lo).max())
    return lo - m, hi + m


# ------------------------------------------------------------------ the families
def inside_out(lo, hi, t0, t1, seed, n=N):
    rng = np.random.default_rng([seed, 1])
    a, b = grown(lo, hi)
    return rtnw.pack_rays(rng.uniform(a, b, (n, 3)), unit(rng, n), 0.001, np.inf, times(rng, n, t0, t1))


def continued(rays1, hits1, on_sphere, seed, n=N):
    """hits1: family 1's result (a dict with prim and t); on_sphere [n]: that hit is on a sphere.
    Also returns, per ray, the primitive it starts on."""
    rng = np.random.default_rng([seed, 2])
    have = hits1["prim"] >= 0
    assert have.any(), "family 1 hit nothing"
    # the hits in turn, odd rays from those on spheres and even rays from those on rects where a scene
    # has both: a sphere can be hit again from inside, a rect only across t = 0
    a, b = np.flatnonzero(have & on_sphere), np.flatnonzero(have & ~on_sphere)
    a, b = (a, b) if len(a) and len(b) else (np.flatnonzero(have),) * 2
    k = np.arange(n)
    at = np.where(k % 2 == 1, a[(k // 2) % len(a)], b[(k // 2) % len(b)])
    o, d, t = rays1["origin"][at], rays1["dir"][at], hits1["t"][at].reshape(-1, 1)
    start = o + t * d
    assert start.dtype == F
    length = F(2.0) ** ((k // 3) % 4)            # |d| of 1, 2, 4, 8: t_min = -0.5 reaches 0.5 to 4 behind the start
    dirs = unit(rng, n).astype(F) * length.reshape(-1, 1).astype(F)
    rays = rtnw.pack_rays(start, dirs, np.array(T_MINS, F)[k % 3], np.inf, rays1["time"][at])
    return rays, hits1["prim"][at]


def _sphere_at(q, kind, time):
    """(centre, radius) of a sphere or of a moving sphere at `time`, float64 (sphere.h:81-83 in exact terms)."""
    if kind == SPHERE:
        return np.array(q[0:3]), abs(q[3])
    c0, c1 = np.array(q[0:3]), np.array(q[3:6])
    return c0 + (time - q[6]) / (q[7] - q[6]) * (c1 - c0), abs(q[8])


def grazing(desc, lo, hi, t0, t1, seed, n=N):
    rng = np.random.default_rng([seed, 3])
    prims = prims_of(desc)
    spheres = [p for p in prims if p.kind <= MSPHERE]
    rects = [p for p in prims if p.kind > MSPHERE]
    n_s = n if not rects else (0 if not spheres else n // 2)
    reach = 0.5 * float(np.linalg.norm(np.subtract(hi, lo, dtype=np.float64)))
    origin, dirs = np.zeros((n, 3), F), np.zeros((n, 3), F)
    time = times(rng, n, t0, t1)
    dd = unit(rng, n)
    dd[0::2, 1] = np.abs(dd[0::2, 1])    # every other ray looks upwards (a chain keeps y): past its target it meets less
    for k in range(n):
        d = dd[k]
        s = reach * (rng.uniform(0.15, 0.6) if k % 2 else rng.uniform(0.02, 0.1))   # the upward ones start close by
        if k < n_s:
            p = spheres[rng.integers(len(spheres))]
            c, r = _sphere_at([float(x) for x in p.p], p.kind, float(time[k]))
            u = np.cross(d, rng.normal(size=3))
            u /= np.linalg.norm(u)
            target = c + r * u                                  # on the silhouette seen along d
        else:
            p = rects[rng.integers(len(rects))]
            a0, a1, b0, b1, kk = (float(x) for x in p.p[0:5])
            j = (k - n_s) % 8                                   # at least one coordinate exactly on an edge
            a = (a0, a0, a1, a1, a0, a1, None, None)[j]
            b = (b0, b1, b0, b1, None, None, b0, b1)[j]
            a = rng.uniform(a0, a1) if a is None else a
            b = rng.uniform(b0, b1) if b is None else b
            ia, ib, ik = {2: (0, 1, 2), 3: (0, 2, 1), 4: (1, 2, 0)}[p.kind]
            target = np.zeros(3)
            target[ia], target[ib], target[ik] = a, b, kk
            u = np.zeros(3)
        ops = chain_of(desc, p)
        o_w, t_w = to_world(ops, target - s * d), to_world(ops, target)
        o32 = o_w.astype(F)                                     # rounded once
        if k < n_s:                                             # 0, +-1, +-4 ulps along u, as the world sees it
            step = (0, 1, -1, 4, -4)[k % 5]
            u_w = to_world(ops, target + u) - t_w
            for _ in range(abs(step)):
                o32 = np.nextafter(o32, np.where(u_w * step > 0, F(np.inf), F(-np.inf)).astype(F))
        origin[k], dirs[k] = o32, (t_w - o_w).astype(F)
    return rtnw.pack_rays(origin, dirs, 0.001, np.inf, time)


def bounded(rays1, hits1, lo, hi, t0, t1, seed, bounds_of, n=N):
    rng = np.random.default_rng([seed, 4])
    n1, n2 = (2 * n) // 3, n // 6
    n3 = n - n1 - n2
    a = rays1[:n1].copy()
    a["t_max"] = bounds_of(np.where(hits1["prim"][:n1] >= 0, hits1["t"][:n1], F(1)), np.arange(n1))
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre, radius = 0.5 * (lo64 + hi64), 0.5 * float(np.linalg.norm(hi64 - lo64))
    # from outside towards the box, stopped short of the sphere around it
    out_d = unit(rng, n2)
    dist = radius * rng.uniform(1.5, 3.0, (n2, 1))
    inside = centre + 0.3 * (hi64 - lo64) * rng.uniform(-1, 1, (n2, 3))
    o2 = centre + dist * out_d
    d2 = inside - o2
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    b = rtnw.pack_rays(o2, d2, 0.001, (0.9 * (dist[:, 0] - radius)).astype(F), times(rng, n2, t0, t1))
    # from beyond the box looking away: everything lies at negative t
    out_d = unit(rng, n3)
    dist = radius * rng.uniform(1.2, 2.0, (n3, 1))
    inside = centre + 0.4 * (hi64 - lo64) * rng.uniform(-1, 1, (n3, 3))
    o3 = centre + dist * out_d
    d3 = o3 - inside
    d3 /= np.linalg.norm(d3, axis=1, keepdims=True)
    c = rtnw.pack_rays(o3, d3, (-4.0 * dist[:, 0]).astype(F), np.inf, times(rng, n3, t0, t1))
    return np.concatenate([a, b, c])


def scaled(rays1, n=N):
    half = n // 2
    out = []
    for e in (-20, 20):
        r = rays1[:half].copy()
        r["dir"] = r["dir"] * F(2.0 ** e)
        r["t_min"] = r["t_min"] * F(2.0 ** -e)
        out.append(r)
    return np.concatenate(out)


def all_families(desc, box, seed, trace, bounds_of):
    """{family: rays} of a scene in box = (lo, hi, t0, t1); trace(rays) answers families 1's hits (the
    oracle's), bounds_of is test_gpu_trace's.  Also "starts": the primitives family 2 starts on."""
    lo, hi, t0, t1 = box
    r1 = inside_out(lo, hi, t0, t1, seed)
    h1 = trace(r1)
    kinds = np.array([p.kind for p in prims_of(desc)] + [-1])
    r2, starts = continued(r1, h1, (h1["prim"] >= 0) & (kinds[h1["prim"]] <= MSPHERE), seed)
    return dict(inside_out=r1, continued=r2, grazing=grazing(desc, lo, hi, t0, t1, seed),
                bounded=bounded(r1, h1, lo, hi, t0, t1, seed, bounds_of), scaled=scaled(r1), starts=starts)


# ------------------------------------------------------------------ radiance records
def path_records(rays, seed):
    """rt_path_ray records of rt_ray records (origin, dir, time), the key fields dealt by index."""
    rng = np.random.default_rng([seed, 6])
    n = len(rays)
    pixel = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    sample = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 2 ** 32 - 1], np.uint32)
    pixel[0::7] = edge[(np.arange(len(pixel[0::7])) // 6) % 2]      # 0 and 2^32 - 1 throughout, under every skip
    sample[3::7] = edge[(np.arange(len(sample[3::7])) // 2) % 2]
    skip = np.array(SKIPS, np.uint32)[np.arange(n) % len(SKIPS)]
    return rtnw.pack_path_rays(rays["origin"], rays["dir"], rays["time"], pixel, sample, skip)


def hand_placed(desc, seed, per=16):
    """(records, labels): `per` rays from inside every dielectric sphere, from inside every
    medium's boundary (its first primitive, or its rects' common box) and from a point on every
    light, in all directions; labels name the kind of each record's start."""
    rng = np.random.default_rng([seed, 7])
    c = desc.contents
    t0, t1 = float(c.time0), float(c.time1)
    starts = []      # (label, ops, f(time) -> point in the primitive's frame)

    def in_sphere(p, share):
        q = [float(x) for x in p.p]
        u = unit(rng, 1)[0]

        def at(t):
            centre, r = _sphere_at(q, p.kind, t)
            return centre + share * r * u
        return at

    def on_rect(p):
        a0, a1, b0, b1, kk = (float(x) for x in p.p[0:5])
        ia, ib, ik = {2: (0, 1, 2), 3: (0, 2, 1), 4: (1, 2, 0)}[p.kind]
        pt = np.zeros(3)
        pt[ia], pt[ib], pt[ik] = rng.uniform(a0, a1), rng.uniform(b0, b1), kk
        return lambda t: pt

    for p in prims_of(desc):
        kind = c.materials[p.material].kind
        if kind == 2 and p.kind <= MSPHERE:
            starts.append(("glass", chain_of(desc, p), in_sphere(p, 0.5)))
        if kind == 3:
            starts.append(("light", chain_of(desc, p), in_sphere(p, 1.0) if p.kind <= MSPHERE else on_rect(p)))
    bp = prims_of(desc, boundary=True)
    for m in range(c.nmedia):
        b = bp[c.media[m].boundary_first:c.media[m].boundary_first + c.media[m].boundary_count]
        if b[0].kind <= MSPHERE:
            starts.append(("medium", chain_of(desc, b[0]), in_sphere(b[0], 0.5)))
        else:
            corners = np.array([x for p in b for x in prim_corners(p)])
            mid = 0.5 * (corners.min(axis=0) + corners.max(axis=0))
            starts.append(("medium", chain_of(desc, b[0]), lambda t, mid=mid: mid))
    origin, time, labels = [], [], []
    for label, ops, at in starts:
        for t in times(rng, per, t0, t1):
            origin.append(to_world(ops, at(float(t))).astype(F))
            time.append(t)
            labels.append(label)
    if not origin:
        return np.zeros(0, rtnw.PATH_RAY_DTYPE), np.array(labels)
    rays = rtnw.pack_rays(np.array(origin, F), unit(rng, len(origin)), 0.001, np.inf, np.array(time, F))
    return path_records(rays, seed + 1), np.array(labels)


def fixture_rays(fam, n=512):
    """n rays for a reference fixture: n / 5 of each family (all_families' result), every 13th ray
    (13 shares no factor with the periods the families deal their variants by)."""
    k = n // len(FAMILIES)
    rest = n - k * len(FAMILIES)
    return np.concatenate([fam[f][::13][:k] for f in FAMILIES] + [fam["inside_out"][1::13][:rest]])
