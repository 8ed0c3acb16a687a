"""Generated scenes for the descriptor-driven parity tests (test_oracle_desc.py on the CPU,
test_gpu_generated.py on the GPU).

A literal table of cases (CASES) maps, through np.random.default_rng(seed), to scene
descriptors (rtnw.SceneDesc.from_arrays) that reach the structural paths rt_scene_create
chooses among and the twelve built-in scenes do not: both sides of the flat-scan, pre-scan,
LDS-media, medium-cell and LDS-BVH limits, every boundary kind of a medium, instance chains of
every op order, textures and materials on every primitive kind, and the ball waves' fused
in-ball step (ball_*, also under tests/test_gpu_ball_generated.py).  The oracle
(oracle.render_desc) says what the image of each is.

Every case names its TARGET: the primitives, media or textures it exists for.
`build(case, plain=True)` is the same scene with the target primitives and media removed and
the target textures replaced by a grey constant; test_oracle_desc.py requires the two oracle
images to differ, so a case whose target the camera does not see fails before any GPU run.

This is a plain module: nothing here touches a GPU, and the numbers in the table's comments
(BVH node counts, depths) were found with a stand-alone program against build_bvh, as
tests/native/bvh_check.cpp is.
"""
import math
from dataclasses import dataclass, field

import numpy as np

import rtnw

SPHERE, MSPHERE, XY, XZ, YZ = 0, 1, 2, 3, 4
OP_T, OP_R, OP_F = 1, 2, 3


class Builder:
    """Collects a descriptor's arrays; indices are returned as they will stand in it."""

    def __init__(self, rng):
        self.rng = rng
        self.textures, self.materials, self.instances = [], [], []
        self.prims, self.boundary, self.media = [], [], []
        self.images, self.texels = [], bytearray()
        self.t_prims, self.t_media, self.t_textures = set(), set(), set()   # the case's target
        # the scene's own Perlin tables (perlin.h:82-111's shape: unit vectors, three permutations)
        v = rng.normal(size=(256, 3))
        self.ranvec = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        self.perm = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.int32)

    # ---- textures
    def const(self, r, g, b):
        self.textures.append(rtnw.RtTexture(kind=0, even=-1, odd=-1, color=(r, g, b), image=-1))
        return len(self.textures) - 1

    def rand_const(self):
        return self.const(*self.rng.uniform(0.15, 0.95, 3))

    def checker(self, even, odd):
        self.textures.append(rtnw.RtTexture(kind=1, even=even, odd=odd, image=-1))
        return len(self.textures) - 1

    def noise(self, scale):
        self.textures.append(rtnw.RtTexture(kind=2, even=-1, odd=-1, scale=scale, image=-1))
        return len(self.textures) - 1

    def image(self, nx, ny, pad=0):
        """A random nx x ny image `pad` bytes after the previous one's texels."""
        self.texels += bytes(pad)
        self.images.append(rtnw.RtImage(offset=len(self.texels), nx=nx, ny=ny))
        self.texels += self.rng.integers(0, 256, 3 * nx * ny, dtype=np.uint8).tobytes()
        self.textures.append(rtnw.RtTexture(kind=3, even=-1, odd=-1, image=len(self.images) - 1))
        return len(self.textures) - 1

    # ---- materials
    def _mat(self, **kw):
        self.materials.append(rtnw.RtMaterial(**kw))
        return len(self.materials) - 1

    def lambert(self, tex=None):
        return self._mat(kind=0, texture=self.rand_const() if tex is None else tex)

    def metal(self, albedo, fuzz):
        return self._mat(kind=1, texture=-1, albedo=tuple(albedo), fuzz=min(float(fuzz), 1.0))

    def glass(self, ri=1.5):
        return self._mat(kind=2, texture=-1, ref_idx=ri)

    def light(self, tex):
        return self._mat(kind=3, texture=tex)

    def iso(self, tex):
        return self._mat(kind=4, texture=tex)

    def rand_mat(self):
        k = self.rng.integers(0, 10)
        if k < 6:
            return self.lambert()
        if k < 8:
            return self.metal(self.rng.uniform(0.4, 1.0, 3), self.rng.uniform(0, 0.6))
        return self.glass(1.5)

    # ---- instance chains: ops are ("t", x, y, z), ("r", degrees), ("f",); ops[0] outermost
    def chain(self, ops):
        inst = rtnw.RtInstance(nops=len(ops))
        for k, op in enumerate(ops):
            if op[0] == "t":
                inst.ops[k][:] = (OP_T, op[1], op[2], op[3])
            elif op[0] == "r":   # hitable.h:98-101
                rad = np.float32((math.pi / 180.) * op[1])
                inst.ops[k][:] = (OP_R, float(np.sin(rad, dtype=np.float32)), float(np.cos(rad, dtype=np.float32)), 0)
            else:
                inst.ops[k][:] = (OP_F, 0, 0, 0)
        self.instances.append(inst)
        return len(self.instances) - 1

    # ---- primitives (returned, not yet placed: add() / medium() place them)
    @staticmethod
    def _prim(kind, mat, inst, flip, p):
        q = rtnw.RtPrim(kind=kind, material=mat, instance=inst, flip=flip)
        q.p[:len(p)] = [float(x) for x in p]
        return q

    def sphere(self, c, r, mat, inst=-1, flip=0):
        return self._prim(SPHERE, mat, inst, flip, (*c, r))

    def msphere(self, c0, c1, t0, t1, r, mat, inst=-1, flip=0):
        return self._prim(MSPHERE, mat, inst, flip, (*c0, *c1, t0, t1, r))

    def rect(self, kind, a0, a1, b0, b1, k, mat, inst=-1, flip=0):
        return self._prim(kind, mat, inst, flip, (a0, a1, b0, b1, k))

    def box(self, p0, p1, mat, inst=-1):   # box.h:23-34
        (x0, y0, z0), (x1, y1, z1) = p0, p1
        return [self.rect(XY, x0, x1, y0, y1, z1, mat, inst), self.rect(XY, x0, x1, y0, y1, z0, mat, inst, 1),
                self.rect(XZ, x0, x1, z0, z1, y1, mat, inst), self.rect(XZ, x0, x1, z0, z1, y0, mat, inst, 1),
                self.rect(YZ, y0, y1, z0, z1, x1, mat, inst), self.rect(YZ, y0, y1, z0, z1, x0, mat, inst, 1)]

    def add(self, *prims, target=False):
        """Appends surface primitives in list order; returns the first one's index."""
        first = len(self.prims)
        for q in prims:
            for x in (q if isinstance(q, list) else [q]):
                if target:
                    self.t_prims.add(len(self.prims))
                self.prims.append(x)
        return first

    def medium(self, boundary, density, tex, target=False):
        """A constant_medium at this place of the list over `boundary` (a primitive or a list)."""
        b = boundary if isinstance(boundary, list) else [boundary]
        self.media.append(dict(first=len(self.boundary), count=len(b), density=density, material=self.iso(tex),
                               order=len(self.prims)))
        self.boundary += b
        if target:
            self.t_media.add(len(self.media) - 1)
        return len(self.media) - 1

    # ---- the descriptor
    def desc(self, plain=False):
        """plain: the scene without its target (primitives and media dropped, textures greyed)."""
        keep_p = [i for i in range(len(self.prims)) if not (plain and i in self.t_prims)]
        keep_m = [i for i in range(len(self.media)) if not (plain and i in self.t_media)]
        kept = set(keep_p)
        before = np.cumsum([0] + [int(i in kept) for i in range(len(self.prims))])   # kept primitives before place i
        media, boundary = [], []
        for i in keep_m:
            m = self.media[i]
            media.append(rtnw.RtMedium(boundary_first=len(boundary), boundary_count=m["count"], density=m["density"],
                                       material=m["material"], order=int(before[m["order"]])))
            boundary += self.boundary[m["first"]:m["first"] + m["count"]]
        textures = list(self.textures)
        if plain:
            for t in self.t_textures:
                textures[t] = rtnw.RtTexture(kind=0, even=-1, odd=-1, color=(0.5, 0.5, 0.5), image=-1)
        return rtnw.SceneDesc.from_arrays(prims=[self.prims[i] for i in keep_p], boundary_prims=boundary, media=media,
                                          materials=self.materials, textures=textures, instances=self.instances,
                                          images=self.images, image_data=bytes(self.texels), perlin_ranvec=self.ranvec,
                                          perlin_perm=self.perm, time0=0.0, time1=1.0)


# ------------------------------------------------------------------------ scene pieces
def small_spheres(b, n, *, lo=(-4, 0.15, -4), hi=(4, 2.5, 4), r=(0.08, 0.2), avoid=()):
    """n small random spheres in a box, none within `avoid` = [(centre, radius)] balls."""
    out = []
    while len(out) < n:
        c = b.rng.uniform(lo, hi)
        rad = float(b.rng.uniform(*r))
        if any(np.linalg.norm(c - np.asarray(ac)) < ar + rad for ac, ar in avoid):
            continue
        out.append(b.sphere(c, rad, b.rand_mat()))
    return out


def ground(b, y=0.0, half=6.0, mat=None):
    return b.rect(XZ, -half, half, -half, half, y, b.lambert(b.checker(b.const(0.2, 0.3, 0.1), b.const(0.9, 0.9, 0.9)))
                  if mat is None else mat)


def mixed_prims(b, n, chains):
    """n primitives of all five kinds at random places, under random ones of `chains` (or none)."""
    out = []
    for i in range(n):
        inst = int(b.rng.choice(chains)) if len(chains) and b.rng.random() < 0.5 else -1
        c = b.rng.uniform((-3, 0.3, -3), (3, 2.5, 3))
        kind = i % 5
        m = b.rand_mat()
        if kind == SPHERE:
            out.append(b.sphere(c, b.rng.uniform(0.2, 0.45), m, inst))
        elif kind == MSPHERE:
            out.append(b.msphere(c, c + b.rng.uniform(-0.3, 0.3, 3), 0.0, 1.0, b.rng.uniform(0.2, 0.4), m, inst))
        else:
            w, h = b.rng.uniform(0.3, 0.9, 2)
            ax = {XY: (0, 1, 2), XZ: (0, 2, 1), YZ: (1, 2, 0)}[kind]
            out.append(b.rect(kind, c[ax[0]] - w, c[ax[0]] + w, c[ax[1]] - h, c[ax[1]] + h, c[ax[2]], m, inst,
                              int(b.rng.integers(0, 2))))
    return out


def ties(b, inst=-1):
    """List-order ties: an exact duplicate sphere with another material, a duplicate moving
    sphere, and coplanar overlapping rects of each kind (aarect.h:50 accepts t == t_max, so
    the LATER of two coplanar rects wins; sphere.h:33 does not, so the EARLIER sphere wins)."""
    red, blue, green = (b.lambert(b.const(*c)) for c in ((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), (0.1, 0.9, 0.1)))
    return [b.sphere((-1.5, 1.0, 1.5), 0.5, red, inst), b.sphere((-1.5, 1.0, 1.5), 0.5, blue, inst),
            b.msphere((1.5, 1.0, 1.5), (1.7, 1.2, 1.5), 0.0, 1.0, 0.4, green, inst),
            b.msphere((1.5, 1.0, 1.5), (1.7, 1.2, 1.5), 0.0, 1.0, 0.4, red, inst),
            b.rect(XY, -0.8, 0.4, 0.3, 1.3, 1.0, red, inst), b.rect(XY, -0.4, 0.8, 0.5, 1.6, 1.0, blue, inst),
            b.rect(XZ, -0.8, 0.4, 1.5, 2.5, 0.25, green, inst), b.rect(XZ, -0.4, 0.8, 1.8, 2.8, 0.25, red, inst),
            b.rect(YZ, 0.3, 1.3, 1.2, 2.2, 2.5, blue, inst, 1), b.rect(YZ, 0.6, 1.6, 1.5, 2.6, 2.5, green, inst, 1)]


# ------------------------------------------------------------------------------- cases
def scan_mixed(b, n):
    """n primitives of mixed kinds, some under one of three chains, the ties among them."""
    chains = [b.chain([("t", 0.5, 0.2, -0.5), ("r", 25.0)]), b.chain([("r", -40.0)]),
              b.chain([("t", -0.7, 0.0, 0.3), ("f",), ("r", 10.0)])]
    t = ties(b) + ties(b, chains[0])
    b.add(ground(b))
    b.add(*mixed_prims(b, n - 1 - len(t), chains)[:n - 1 - len(t)])
    b.add(*t, target=True)


def scan_spheres(b, n=64):
    """n spheres, no chain: one group holding 64 primitives of one kind."""
    b.add(b.sphere((0, -100, 0), 100, b.lambert()))
    b.add(*small_spheres(b, n - 5, lo=(-3, 0.2, -3), hi=(3, 2.5, 3), r=(0.15, 0.35)))
    b.add(*[q for q in ties(b) if q.kind == SPHERE], b.sphere((0, 1.2, 2.0), 0.4, b.glass()),
          b.sphere((0, 1.2, 2.0), -0.35, b.glass()), target=True)


def scan_own_chains(b, n=64):
    """n primitives, each under a chain index of its own: one group per primitive.  The last
    ten are ties(): every member of a duplicate or coplanar pair under a separate chain of the
    SAME ops, so the two stand in different scan groups at the same world place and the scan
    (sorted by chain, then kind) must still return the (t, list order) winner."""
    for i in range(n - 10):
        ops = [("t", *b.rng.uniform(-0.4, 0.4, 3)), ("r", float(b.rng.uniform(-30, 30)))]
        q = mixed_prims(b, 5, [])[i % 5]
        q.instance = b.chain(ops[:1 + i % 2])
        b.add(q, target=True)
    same = [("t", 0.2, 0.1, -0.3), ("r", 20.0)]
    for q in ties(b):
        q.instance = b.chain(same)
        b.add(q, target=True)


def scan_five_kinds(b):
    """One chain shared by primitives of all five kinds (one group, five runs) + the ties under it."""
    c = b.chain([("t", 0.3, 0.1, -0.2), ("r", 30.0)])
    qs = mixed_prims(b, 10, [])
    for q in qs:
        q.instance = c
    b.add(*qs, *ties(b, c), target=True)


def prescan(b, nbig):
    """80 small spheres and nbig primitives above 10 % of the scene box's area (a rect, an
    instanced rect, a moving sphere, spheres; two are duplicates).  The scene box is the
    ground's 12 x 12 up to the instanced rect's y = 4: area 2 (144 + 2 * 12 * 4) = 480, 10 % = 48."""
    c = b.chain([("t", 0.0, 0.0, -5.0), ("r", 0.0)])
    big = [ground(b),                                                               # 288
           b.rect(XY, -6, 6, 0, 4, 0.0, b.lambert(), c),                            # 96, instanced
           b.msphere((-3, 1.6, 0), (-2.4, 1.6, 0), 0, 1, 1.6, b.lambert()),         # 3.8 x 3.2 x 3.2: 69
           b.sphere((3, 1.5, -1), 1.5, b.metal((0.8, 0.8, 0.8), 0.1)),              # 54
           b.sphere((0.5, 1.5, -2.5), 1.5, b.lambert(b.const(0.9, 0.2, 0.2))),      # 54
           b.sphere((0.5, 1.5, -2.5), 1.5, b.lambert(b.const(0.2, 0.2, 0.9))),      # its duplicate
           b.sphere((-0.5, 1.48, 2), 1.48, b.glass()),                              # 52.6
           b.sphere((2.5, 1.46, 2.5), 1.46, b.lambert()),                           # 51.2
           b.sphere((-3.5, 1.44, 3.5), 1.44, b.lambert(b.const(0.9, 0.9, 0.1)))]    # 49.8 >= 48: the ninth candidate, the
    #                                                                  smallest: the cap of 8 leaves it in the BVH
    small = small_spheres(b, 80, avoid=[(q.p[0:3], abs(q.p[3])) for q in big if q.kind == SPHERE] +
                          [((-2.7, 1.6, 0), 1.9)])
    # the big ones spread through the list: the pre-scan keeps list order as the tie order
    step = len(small) // nbig
    for k in range(nbig):
        b.add(*small[k * step:(k + 1) * step])
        b.add(big[k], target=True)
    b.add(*small[nbig * step:])


def media_count(b, nmedia, bvh):
    """nmedia overlapping spherical media of distinct densities and colours in two rows; the
    media from the ninth on (index >= RT_LDS_MEDIA = 8) stand in front, away from the others."""
    b.add(ground(b))
    if bvh:
        b.add(*small_spheres(b, 70, lo=(-4, 0.1, -4), hi=(4, 0.5, 0), r=(0.05, 0.12)))
    else:
        b.add(*small_spheres(b, 6, lo=(-3, 0.2, -3), hi=(3, 0.6, 0), r=(0.1, 0.2)))
    glass = b.glass()
    for k in range(nmedia):
        late = k >= 8
        c = ((k - 9.5) * 1.1, 0.7, 2.6) if late else ((k - 3.5) * 0.8, 1.0, 0.4 * (k % 2))
        b.medium(b.sphere(c, 0.5 if late else 0.7, glass), 0.6 + 0.45 * k, b.rand_const(), target=late or nmedia <= 8)


def boundary_kinds(b, bvh):
    """Media bounded by a moving sphere, an instanced sphere (count 1, instance >= 0: not the
    fast path), two spheres, a box under a 6-op chain and a negative-radius sphere."""
    b.add(ground(b))
    if bvh:
        b.add(*small_spheres(b, 70, lo=(-4, 0.1, -4), hi=(4, 0.4, -1), r=(0.05, 0.12)))
    g = b.glass()
    b.medium(b.msphere((-3, 1, 0), (-2.6, 1.3, 0), 0, 1, 0.7, g), 1.5, b.const(0.9, 0.2, 0.2), target=True)
    b.medium(b.sphere((0, 0, 0), 0.7, g, b.chain([("t", -1.2, 1.0, 0.5), ("r", 30.0)])), 2.0, b.const(0.2, 0.9, 0.2),
             target=True)
    b.medium([b.sphere((0.2, 1.0, 0), 0.6, g), b.sphere((0.9, 1.2, 0.2), 0.5, g)], 2.5, b.const(0.2, 0.2, 0.9),
             target=True)
    six = b.chain([("t", 2.2, 0.2, 0.0), ("r", 20.0), ("t", 0.1, 0.0, 0.1), ("f",), ("r", -35.0), ("t", -0.5, 0, -0.5)])
    b.medium(b.box((0, 0, 0), (1, 1.4, 1), g, six), 3.0, b.const(0.9, 0.9, 0.2), target=True)
    b.medium(b.sphere((3.4, 0.9, 1.0), -0.7, g), 1.0, b.const(0.9, 0.5, 0.9), target=True)


def cell(b, variant):
    """Medium-cell and deep-first claims on a BVH scene (> 64 primitives)."""
    g = b.glass()
    balls = {   # (centre, radius, density): the candidates; reach = R + R / 64 + 1e-3 |c|max
        "two_dense": [((-1.5, 1.0, 0), 0.9, 8.0), ((1.5, 1.0, 0), 0.9, 20.0)],
        "two_equal": [((-1.5, 1.0, 0), 0.9, 12.0), ((1.5, 1.0, 0), 0.9, 12.0)],
        "near4": [((0, 1.3, 0), 1.0, 10.0)],
        "near5": [((0, 1.3, 0), 1.0, 10.0)],
        "near_inst_moving": [((0, 1.3, 0), 1.0, 10.0)],
        "dup_outside": [((0, 1.3, 0), 1.0, 10.0)],
        "not_dense": [((-1.5, 1.0, 0), 0.9, 2.0), ((1.5, 1.0, 0), 0.9, 9.0)],   # 1/2 >= 0.45: not deep; 1/9 < 0.45
    }[variant]
    b.add(ground(b))   # not a near primitive: every ball floats more than its reach above y = 0
    avoid = [(c, r + 0.45) for c, r, _ in balls]
    b.add(*small_spheres(b, 75, avoid=avoid))
    for c, r, dens in balls:
        shell = b.sphere(c, r, g)
        b.add(shell, target=True)            # the glass shell, as final()'s ball has: near primitive 1
        b.medium(b.sphere(c, r, g), dens, b.rand_const(), target=True)
    c, r, _ = balls[0]
    red = b.lambert(b.const(0.9, 0.1, 0.1))
    inside = [b.sphere((c[0] + 0.3, c[1], c[2]), 0.15, red), b.sphere((c[0] - 0.3, c[1] + 0.2, c[2]), 0.15, b.lambert()),
              b.sphere((c[0], c[1] - 0.3, c[2] + 0.3), 0.15, b.metal((0.9, 0.9, 0.9), 0.0))]
    if variant == "near4":
        b.add(*inside, target=True)          # shell + 3 = 4 = RT_CELL_MAX: the cell is taken
    if variant == "near5":
        b.add(*inside, b.sphere((c[0], c[1] + 0.35, c[2] - 0.3), 0.12, b.lambert()), target=True)   # 5: declined
    if variant == "near_inst_moving":
        ch = b.chain([("t", c[0], c[1], c[2]), ("r", 45.0)])
        b.add(b.sphere((0.35, 0, 0), 0.15, red, ch), b.msphere((c[0] - 0.3, c[1], c[2]), (c[0] - 0.2, c[1] + 0.2, c[2]),
                                                                0, 1, 0.15, b.lambert()),
              b.rect(XY, -0.3, 0.3, -0.2, 0.2, 0.1, b.lambert(), ch, 1), target=True)
    if variant == "dup_outside":   # shell + 2 + an exact duplicate of the red one (4 near), and a copy of it outside the cell
        b.add(*inside[:2], b.sphere((c[0] + 0.3, c[1], c[2]), 0.15, b.lambert(b.const(0.1, 0.9, 0.1))),
              b.sphere((c[0] + 0.3, c[1] + 1.6, c[2]), 0.15, red), target=True)


BALL_R = 1.0
BALL_ALB = ((0.85, 0.55, 0.25), (0.3, 0.6, 0.9), (0.5, 0.8, 0.4))   # the ball's, the second medium's, the third's
# the ball's density by variant (mean free path 1 / density; dense, "deep", where that is below R / 2)
BALL_DENSITY = {"one_medium": 8.0, "dense_first": 6.0, "dense_second": 6.0, "in_fog_on_ground": 3.0, "full_cell": 4.0,
                "thin": 0.5, "negative_radius": 8.0, "solid": 1e30, "three_media": 6.0, "noise_medium": 6.0,
                "with_instance": 6.0, "camera_inside": 4.0}
BALL_QUALIFY = ("one_medium", "dense_first", "dense_second", "in_fog_on_ground", "full_cell", "thin", "negative_radius",
                "solid", "camera_inside")                        # rt_scene_desc_ball_fast = 1, and the step can run
BALL_DECLINE = ("three_media", "noise_medium", "with_instance")  # lowering says 0, 0, 1; the step never runs
BALL_LOOKFROM = (0.0, 1.7, 2.7)
# camera_inside: full_cell seen from inside the ball, so that camera rays, which carry a time of their own, start
# there (behind the glass shell every segment inside the ball has time 0 already: a dielectric leaves it so)
BALL_INSIDE_LOOKFROM = (0.25, 1.45, 0.6)


def ball_centre(variant):
    """in_fog_on_ground's ball floats 0.01 above the ground, less than its margin R / 64 + 1e-3 |c|max = 0.0166."""
    return (0.0, BALL_R + 0.01, 0.0) if variant == "in_fog_on_ground" else (0.0, 1.3, 0.0)


def ball(b, variant):
    """The ball waves' fused in-ball step (rt_megakernel.h stage 3) on a BVH scene of more than 64
    primitives without an instance chain: one dense sphere-bounded ball of radius BALL_R that
    fills most of the frame, every medium an isotropic of a constant texture (BALL_ALB: distinct,
    no component 0 or 1), the ground and 77 small spheres out of the ball's reach."""
    c, R, dens = ball_centre(variant), BALL_R, BALL_DENSITY[variant]
    g = b.glass()
    second = np.add(c, (0.6, 0.0, 0.0))   # the second medium's sphere (radius R): the lens is 56 % of the ball
    avoid = [(c, R + 0.45), (second, R + 0.45), (BALL_LOOKFROM, 0.6)]
    third_c, box_at = (3.0, 0.7, -1.5), (3.0, 0.0, -2.0)
    if variant == "three_media":
        avoid.append((third_c, 0.5 + 0.3))
    if variant == "with_instance":
        avoid.append((np.add(box_at, (0.3, 0.3, 0.3)), 1.0))
    # The ball waves exist only in the kernel variant of the feature set "media" alone (rt_megakernel.h kBall):
    # no checker texture, no pre-scanned primitive, no instance chain.  So the ground is a plain 4.8 x 4.8
    # lambertian (box area 46) and the scene box is pinned to 12 x 5.8 x 12 by two spheres in its corners
    # (area 566): neither the ground nor the ball's shell (24) reaches the pre-scan's 10 % of it.
    # The ground is not a near primitive, except in in_fog_on_ground
    b.add(ground(b, half=2.4, mat=b.lambert(b.const(0.5, 0.5, 0.45))))
    b.add(b.sphere((-5.9, 0.3, -5.9), 0.1, b.lambert()), b.sphere((5.9, 5.9, 5.9), 0.1, b.lambert()))
    if variant == "in_fog_on_ground":
        # spheres of radius 0.2 whose boxes stay just outside the ball's reach R + 0.0166 (the rule measures
        # boxes: a corner is up to 0.2 sqrt(3) nearer than the centre): a ring resting on the ground at 1.15
        # from the axis and one at the ball's height at 1.34.  A ray that leaves the ball downwards meets one
        # of them, or a fog scatter, before the ground
        ring = [b.sphere((1.15 * math.cos(a), 0.22, 1.15 * math.sin(a)), 0.2, b.rand_mat())
                for a in np.arange(16) * (2 * math.pi / 16)]
        ring += [b.sphere((1.34 * math.cos(a), c[1], 1.34 * math.sin(a)), 0.2, b.rand_mat())
                 for a in (np.arange(16) + 0.5) * (2 * math.pi / 16) if math.sin(a) < 0.7]   # (not in the camera's way)
        b.add(*ring, target=True)
        avoid[0] = (c, R + 0.75)
    b.add(*small_spheres(b, 75, lo=(-5, 0.15, -5), hi=(5, 4.0, 5), avoid=avoid))
    rb = -R if variant == "negative_radius" else R

    def the_ball():
        if variant != "in_fog_on_ground":
            b.add(b.sphere(c, rb, g), target=True)   # the glass shell: near primitive 1
        b.medium(b.sphere(c, rb, g), dens, b.const(*BALL_ALB[0]), target=True)

    def the_second():
        tex = b.noise(4.0) if variant == "noise_medium" else b.const(*BALL_ALB[1])
        # mean free path 1 / 1.5 = 0.67 R against the ball's 1 / 6: in the lens it scatters a fifth of the segments
        b.medium(b.sphere(second, R, g), 1.5, tex, target=True)

    if variant in ("dense_first", "three_media", "noise_medium", "with_instance"):
        the_ball()      # the cell goes to medium 0: the ball, the first candidate of the greatest density
        the_second()
    elif variant == "dense_second":
        the_second()    # medium 0 is a candidate too (the shell is its one near primitive), and
        the_ball()      # the cell goes to medium 1: the ball, of strictly greater density
    else:
        the_ball()
    if variant == "in_fog_on_ground":   # a scene-wide fog of mean free path 12.5, the ground's side 12; no cell candidate
        b.medium(b.sphere((0.0, 0.0, 0.0), 30.0, g), 0.08, b.const(*BALL_ALB[1]), target=True)
    if variant == "three_media":
        b.medium(b.sphere(third_c, 0.5, g), 2.0, b.const(*BALL_ALB[2]))
    if variant == "with_instance":   # far from the ball: the kernel variant with instance chains has no ball waves
        b.add(*b.box((0, 0, 0), (0.6, 0.6, 0.6), b.lambert(), b.chain([("t", *box_at), ("r", 30.0)])))
    if variant in ("full_cell", "camera_inside"):   # the shell + 3 inside the ball = RT_CELL_MAX near primitives
        b.add(b.sphere((c[0] + 0.4, c[1], c[2]), 0.2, b.metal((0.9, 0.8, 0.7), 0.0)),
              b.msphere((c[0] - 0.4, c[1] - 0.15, c[2] + 0.1), (c[0] - 0.4, c[1] + 0.2, c[2] + 0.1), 0, 1, 0.15,
                        b.lambert(b.const(0.9, 0.1, 0.1))),     # centres 0.35 apart, radius 0.15
              b.rect(XZ, c[0] - 0.4, c[0] + 0.4, c[2] - 0.4, c[2] + 0.4, c[1] - 0.5, b.lambert(b.const(0.2, 0.8, 0.3))),
              target=True)


def _op(b, kind):
    if kind == "t":
        return ("t", *b.rng.uniform(-0.35, 0.35, 3))
    if kind == "r":
        return ("r", float(b.rng.uniform(-60, 60)))
    return ("f",)


def _chain_prim(b, i, inst, c):
    """Object number i under chain inst near c: sphere, moving sphere, rects in turn."""
    m = b.lambert() if i % 3 else b.rand_mat()
    kind = i % 5
    if kind == SPHERE:
        return b.sphere(c, 0.28, m, inst)
    if kind == MSPHERE:
        return b.msphere(c, c + np.array((0.15, 0.1, 0.0)), 0, 1, 0.25, m, inst)
    ax = {XY: (0, 1, 2), XZ: (0, 2, 1), YZ: (1, 2, 0)}[kind]
    return b.rect(kind, c[ax[0]] - 0.3, c[ax[0]] + 0.3, c[ax[1]] - 0.3, c[ax[1]] + 0.3, c[ax[2]], m, inst, i % 2)


def chains_short(b):
    """Every op order of length 1 to 3 (3 + 9 + 27 chains), one primitive under each."""
    import itertools
    b.add(ground(b, y=-0.5))
    i = 0
    for n in (1, 2, 3):
        for kinds in itertools.product("trf", repeat=n):
            c = np.array(((i % 8 - 3.5) * 0.8, 0.3 + (i // 8) * 0.55, -1.0 + (i % 3) * 0.6))
            b.add(_chain_prim(b, i, b.chain([_op(b, k) for k in kinds]), c), target=True)
            i += 1


def chains_long(b):
    """Chains of 4 to 6 ops (sampled), FLIP at the first, middle and last place, under spheres
    carrying an image texture and under moving spheres; one chain shared by many primitives,
    and identical chains under different indices."""
    b.add(ground(b, y=-0.5))
    img = b.lambert(b.image(7, 5))
    b.t_textures.add(len(b.textures) - 1)
    i = 0
    for n in (4, 5, 6):
        for flip_at in (0, n // 2, n - 1, None):
            kinds = [str(b.rng.choice(list("tr"))) for _ in range(n)]
            if flip_at is not None:
                kinds[flip_at] = "f"
            inst = b.chain([_op(b, k) for k in kinds])
            c = np.array(((i % 6 - 2.5) * 1.0, 0.3 + (i // 6) * 0.9, -0.5))
            q = b.sphere(c, 0.33, img, inst) if i % 2 == 0 else b.msphere(c, c + np.array((0.2, 0.1, 0)), 0, 1, 0.3,
                                                                          b.lambert(), inst)
            b.add(q, target=True)
            i += 1
    ops = [("t", 0.0, 0.0, 1.6), ("r", 33.0), ("f",), ("t", 0.1, 0.0, 0.0)]
    shared = b.chain(ops)
    for k in range(12):   # one chain, many primitives (one scan group)
        b.add(_chain_prim(b, k, shared, np.array(((k - 5.5) * 0.55, 0.2 + 0.1 * (k % 3), 0.0))), target=True)
    for k in range(6):    # the same ops again under indices of their own
        b.add(_chain_prim(b, k, b.chain(ops), np.array(((k - 2.5) * 0.9, 1.3, 0.3))), target=True)


def textures_by_kind(b):
    """Image textures on each rect kind and on an instanced sphere, two images at different
    offsets and sizes (1 x 1 included), a checker nested to depth 15, noise on an instanced
    rect, metal (fuzz 0 and 1) and dielectric rects and boxes, a textured light."""
    im_a, im_b = b.image(9, 6), b.image(1, 1, pad=5)
    chk = b.const(0.9, 0.9, 0.9)
    for k in range(15):   # depth 15: the leaf is 15 checkers down (validate_desc allows no more)
        chk = b.checker(chk, b.const(*((0.1 + 0.05 * k, 0.8 - 0.05 * k, 0.3) if k % 2 else (0.8, 0.1 + 0.04 * k, 0.2))))
    noise = b.noise(3.0)
    b.t_textures |= {im_a, im_b, chk, noise}
    b.add(b.rect(XZ, -6, 6, -6, 6, 0.0, b.lambert(chk)))
    ch = b.chain([("t", -2.5, 1.0, 0.5), ("r", 40.0)])
    b.add(b.rect(XY, -3.5, -2.0, 1.6, 2.8, -1.0, b.lambert(im_a)), b.rect(XZ, -0.8, 0.8, 0.5, 2.0, 0.02, b.lambert(im_a)),
          b.rect(YZ, 0.2, 1.6, -1.0, 1.0, 3.2, b.lambert(im_a), -1, 1), b.sphere((0, 0, 0), 0.6, b.lambert(im_a), ch),
          b.sphere((-1.0, 0.5, 1.0), 0.5, b.lambert(im_b)), b.rect(XY, 2.0, 3.0, 1.8, 2.8, -1.0, b.lambert(im_b)))
    b.add(b.rect(XY, -1.0, 1.0, -0.5, 1.0, 0.0, b.lambert(noise), b.chain([("t", 0.0, 1.2, -1.5), ("r", -20.0)])))
    b.add(b.rect(XY, -1.9, -0.4, 0.3, 1.5, -0.8, b.metal((0.9, 0.8, 0.7), 0.0)),
          b.rect(YZ, 0.2, 1.4, -0.6, 0.8, -3.3, b.metal((0.7, 0.8, 0.9), 1.0)),
          b.rect(XZ, 1.0, 2.2, 0.8, 2.0, 0.6, b.glass()), target=True)
    b.add(*b.box((1.2, 0.0, -0.8), (2.2, 1.0, 0.2), b.glass(), b.chain([("r", 15.0)])),
          *b.box((-0.3, 0.02, 2.2), (0.5, 0.6, 3.0), b.metal((0.9, 0.9, 0.9), 0.0)),
          *b.box((2.4, 0.0, 1.2), (3.2, 0.7, 2.0), b.metal((0.9, 0.6, 0.3), 1.0)), target=True)
    b.add(b.rect(XZ, -2, 2, -2, 2, 4.5, b.light(b.checker(b.const(6, 6, 6), b.const(6, 1, 1))), -1, 1),
          b.sphere((2.8, 2.2, 0.5), 0.4, b.light(im_a)), target=True)


def image_rects(b):
    """An image texture on an xy, an xz and a yz rect, plain and flipped, under the sky: the
    texel a lambertian hit reads decides the pixel (in textures_by_kind's closed room most
    paths end in black whatever the texel was)."""
    im = b.image(9, 6)
    b.t_textures.add(im)
    for flip, dx in ((0, -2.2), (1, 1.2)):
        b.add(b.rect(XY, dx - 0.8, dx + 0.6, 0.2, 1.6, -0.5, b.lambert(im), -1, flip),
              b.rect(XZ, dx - 0.6, dx + 0.8, 0.0, 1.8, 0.1, b.lambert(im), -1, flip),
              b.rect(YZ, 0.2, 1.6, -0.5, 1.5, dx + 1.0, b.lambert(im), -1, flip), target=True)


def cloud(b, n, extra=None, copies=1):
    """A uniform cloud of n small spheres (extra: "cell_prescan" adds, within the n, a ground
    rect and a large sphere for the pre-scan and a dense ball with a shell for the cell).
    copies > 1: every sphere stands `copies` times in a row, each copy with a material of its
    own: the builder's leaves fill up (n primitives in about n / copies nodes), and every hit
    is a list-order tie."""
    k = n
    if extra == "cell_prescan":
        g = b.glass()
        b.add(b.rect(XZ, -6, 6, -6, 6, 0.0, b.lambert()), b.sphere((3.0, 1.6, -3.0), 1.6, b.lambert()), target=True)
        b.add(b.sphere((0, 1.2, 2.5), 0.8, g), target=True)
        b.medium(b.sphere((0, 1.2, 2.5), 0.8, g), 10.0, b.const(0.9, 0.3, 0.2), target=True)
        k = n - 3
        avoid = [((0, 1.2, 2.5), 1.3), ((3.0, 1.6, -3.0), 1.7)]
    else:
        avoid = []
    sites = small_spheres(b, -(-k // copies), lo=(-4, 0.2, -4), hi=(4, 3.5, 4), r=(0.03, 0.09), avoid=avoid)
    out = []
    for q in sites:
        out.append(q)
        out += [b.sphere(q.p[0:3], q.p[3], b.lambert()) for _ in range(copies - 1)]
    b.add(*out[:k], target=extra is None)


def progression(b, n=200):
    """A geometric progression of n spheres: centres and radii grow by a constant factor, so
    every median split leaves one side far larger than the other's extent."""
    q = 1.2
    for k in range(n):
        s = q ** k
        b.add(b.sphere((1e-3 * s, 1e-3 * s * 0.5, -1e-3 * s * 0.3), 2.5e-4 * s, b.rand_mat()), target=k % 2 == 0)


@dataclass
class Case:
    name: str
    make: object            # f(builder)
    seed: int
    nx: int = 24
    ny: int = 16
    spp: int = 4
    max_depth: int = 50
    background: str = "sky"
    lookfrom: tuple = (0.0, 2.6, 9.0)
    lookat: tuple = (0.0, 0.9, 0.0)
    vfov: float = 40.0
    aperture: float = 0.05
    expect: dict = field(default_factory=dict)   # rt_stats fields of the default build
    knobs: tuple = ()       # the RTNW_* knobs that change this scene's path ("RTNW_SCAN", ...)

    def builder(self):
        b = Builder(np.random.default_rng(self.seed))
        self.make(b)
        return b

    def camera(self):
        aspect = float(np.float32(self.nx) / np.float32(self.ny))
        focus = float(np.linalg.norm(np.subtract(self.lookfrom, self.lookat)))
        return rtnw.Camera(self.lookfrom, self.lookat, (0, 1, 0), self.vfov, aspect, self.aperture, focus, 0.0, 1.0)


def _c(name, make, seed, **kw):
    return Case(name=name, make=make, seed=seed, **kw)


SCAN = ("RTNW_SCAN",)
BVH = ("RTNW_LDS_BVH",)
FAR = dict(lookfrom=(0.0, 5.0, 13.0), lookat=(0.0, 1.0, 0.0))

BIG = dict(nx=16, ny=8, spp=2)   # the scenes of thousands of primitives

CASES = [
    # 1. flat-scan boundary (RT_SCAN_MAX = 64); scan_groups = the number of distinct chains
    _c("scan64_mixed", lambda b: scan_mixed(b, 64), 101, expect=dict(scan_groups=4, prescan=0), knobs=SCAN),
    _c("scan65_mixed", lambda b: scan_mixed(b, 65), 101, expect=dict(scan_groups=0), knobs=BVH),
    _c("scan64_spheres", scan_spheres, 103, expect=dict(scan_groups=1), knobs=SCAN),
    _c("scan64_own_chains", scan_own_chains, 104, max_depth=6, expect=dict(scan_groups=64), knobs=SCAN),
    _c("scan_five_kinds", scan_five_kinds, 105, expect=dict(scan_groups=1), knobs=SCAN),
    # 2. pre-scan (RT_PRESCAN_MAX = 8): 80 small + 1, 8, 9 large primitives
    _c("prescan1", lambda b: prescan(b, 1), 201, expect=dict(scan_groups=0, prescan=1), knobs=BVH + ("RTNW_PRESCAN",), **FAR),
    _c("prescan8", lambda b: prescan(b, 8), 202, expect=dict(prescan=8), knobs=BVH + ("RTNW_PRESCAN",), **FAR),
    _c("prescan9", lambda b: prescan(b, 9), 203, max_depth=6, expect=dict(prescan=8), knobs=BVH + ("RTNW_PRESCAN",), **FAR),
    # 3. media count either side of RT_LDS_MEDIA = 8
    _c("media8_scan", lambda b: media_count(b, 8, False), 301, expect=dict(scan_groups=1), knobs=SCAN),
    _c("media9_scan", lambda b: media_count(b, 9, False), 302, expect=dict(scan_groups=1), knobs=SCAN),
    _c("media12_scan", lambda b: media_count(b, 12, False), 303, max_depth=6, expect=dict(scan_groups=1), knobs=SCAN),
    _c("media9_bvh", lambda b: media_count(b, 9, True), 304, expect=dict(scan_groups=0, prescan=1),
       knobs=BVH + ("RTNW_PRESCAN", "RTNW_CELL")),   # (its densest plain ball gets a cell: test_oracle_desc cell_choice)
    _c("media12_bvh", lambda b: media_count(b, 12, True), 305, expect=dict(scan_groups=0, prescan=1),
       knobs=BVH + ("RTNW_PRESCAN", "RTNW_CELL")),
    # 4. boundary kinds
    _c("boundaries_scan", lambda b: boundary_kinds(b, False), 401, spp=8, expect=dict(scan_groups=1), knobs=SCAN),
    _c("boundaries_bvh", lambda b: boundary_kinds(b, True), 402, spp=8, expect=dict(scan_groups=0), knobs=BVH + ("RTNW_PRESCAN",)),
    # 5. medium cell (RT_CELL_MAX = 4) and deep-first claims
    *[_c(f"cell_{v}", (lambda v: lambda b: cell(b, v))(v), 500 + i, expect=dict(scan_groups=0),
         knobs=BVH + ("RTNW_PRESCAN", "RTNW_CELL"), lookfrom=(0.0, 2.0, 6.5), lookat=(0.0, 1.0, 0.0))
      for i, v in enumerate(("two_dense", "two_equal", "near4", "near5", "near_inst_moving", "dup_outside", "not_dense"))],
    # 5b. the ball waves' fused in-ball step: the variants that run it, then those that must not
    *[_c(f"ball_{v}", (lambda v: lambda b: ball(b, v))(v), 900 + i, nx=48, ny=32, spp=8,
         max_depth=8 if v == "solid" else 50, expect=dict(scan_groups=0, lds_level=1, prescan=0),
         knobs=BVH + ("RTNW_PRESCAN", "RTNW_CELL"), lookfrom=BALL_LOOKFROM, lookat=ball_centre(v))
      for i, v in enumerate(BALL_QUALIFY[:8] + BALL_DECLINE)],
    _c("ball_camera_inside", lambda b: ball(b, "camera_inside"), 911, nx=48, ny=32, spp=8, expect=dict(scan_groups=0, lds_level=1, prescan=0),
       knobs=BVH + ("RTNW_PRESCAN", "RTNW_CELL"), lookfrom=BALL_INSIDE_LOOKFROM, lookat=(-0.4, 1.32, 0.1), vfov=70.0),
    # 6. LDS-resident BVH limits: nnodes <= 1024, nprims < 4096, stack = depth + 1 (node counts and
    #    depths from build_bvh, run stand-alone on these very primitives)
    _c("cloud1732", lambda b: cloud(b, 1732), 601, **BIG, expect=dict(lds_level=1, stack_depth=13), knobs=BVH),   # 1024 nodes
    _c("cloud1736", lambda b: cloud(b, 1736), 601, **BIG, expect=dict(lds_level=0), knobs=()),                    # 1030 nodes
    _c("quad4095", lambda b: cloud(b, 4095, copies=4), 606, **BIG, expect=dict(lds_level=1), knobs=BVH),
    _c("quad4096", lambda b: cloud(b, 4096, copies=4), 606, **BIG, expect=dict(lds_level=0), knobs=()),
    _c("quad4095_cell_prescan", lambda b: cloud(b, 4095, "cell_prescan", copies=4), 607, **BIG,
       expect=dict(lds_level=1, prescan=2), knobs=BVH + ("RTNW_PRESCAN", "RTNW_CELL")),
    _c("cloud1800_cell_prescan", lambda b: cloud(b, 1800, "cell_prescan"), 608, **BIG,   # 1069 nodes: HBM, with pre-scan and cell
       expect=dict(lds_level=0, prescan=2), knobs=("RTNW_PRESCAN", "RTNW_CELL")),
    _c("progression200", progression, 605, nx=16, ny=8, spp=2, lookfrom=(0.0, 0.0, 1.0), lookat=(0.5, 0.25, -0.15),
       vfov=70.0, aperture=0.0, expect=dict(stack_depth=23), knobs=BVH),
    # 7. instance chains
    _c("chains_short", chains_short, 701, expect=dict(scan_groups=40), knobs=SCAN),
    _c("chains_long", chains_long, 702, max_depth=6, expect=dict(scan_groups=20), knobs=SCAN),
    # 8. textures and materials by primitive kind
    _c("image_rects", image_rects, 802, expect=dict(scan_groups=1), knobs=SCAN, lookfrom=(-1.5, 2.5, 7.0),
       lookat=(0.0, 0.8, 0.0)),
    _c("textures_by_kind", textures_by_kind, 801, spp=8, background="black", expect=dict(scan_groups=4), knobs=SCAN),
]

BY_NAME = {c.name: c for c in CASES}


def build(case, plain=False):
    """(SceneDesc, Camera) of a case; plain: without the case's target."""
    return case.builder().desc(plain), case.camera()
