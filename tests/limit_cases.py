"""The case table of the parity tests at the ABI's numeric limits (include/rt_hip.h,
rt_render_params): test_limits_spec.py on the CPU, test_gpu_limits.py on the GPU.

Frames of 65535 x 65535 pixels, the largest the ABI takes, rendered a tile at a time: 8 x 8
tiles in the four corners and at the centre, the four corner pixels and two full strips.  The
centre tile holds row j = 32768 (image row 32766) and column 32768, where the pixel key
j * nx + x reaches 2^31; from j = 32769 on, the upper half of the frame, j * nx alone passes
INT_MAX.  Beside the frames: the last legal sample indices, seeds with the top bit set, and
chunks up to INT_MAX.

A case must be able to fail.  A far tile of such a frame sees almost one direction, and a
wrong pixel key only shows where two pixels' radiances differ, so test_limits_spec.py holds
every case to `powerful`: at least half of the oracle's pixels nonzero and no two nonzero
pixels bit-equal.  The frames below are chosen for that:

  * every frame has the sky background.  cornell_box and final are lit by one small lamp; under
    their own black background 2-30 % of a far tile's pixels are nonzero at 4 spp, and those are
    products of a few constant albedos and the lamp's 15, equal in many pixels.  The sky
    makes every escaping path's radiance a function of its last direction.  The scenes'
    structural paths do not depend on the background (cornell_box: flat scan, no libm call;
    final: media, deep-first claims, ball waves; random_scene: the BVH in LDS);
  * cornell_box and final are seen through the `final_alt` preset (vfov 20 from inside the
    box's opening): every pixel of the frame, the corners too, looks at surfaces inside the
    scene.  Under the `cornell` preset the corners of a square frame look past the box, and a
    tile of primary rays into the sky is a tile of near-equal colours.

The strips are held to `powerful_strip` instead, and that is a deliberate difference: a
sample's radiance is a product of constant albedos and either the lamp's constant or
sky(t), t one float32 in [0.5, 1), so one-sample pixels take fewer than 2^23 values per
albedo product and 65535 of them hold 65535^2 / 2 / 2^23 = 256 equal pairs by the birthday
bound, whatever the strip (measured on these frames: 87 to 8485).  A strip must have at
least half its pixels nonzero AND bitwise unique in the strip: a key error that moves more
than a few pixels cannot hide there either.

Nothing here touches a GPU.
"""
from dataclasses import dataclass

import numpy as np

import oracle as O
import rtnw

N = 65535                       # nx = ny of every frame
T = 8                           # the tile size
LAST = 0xFFFFFFFF               # sample_offset + spp may reach this, not pass it

# scene -> the frame's camera preset, background and depth (the scenes' own depths)
FRAMES = {
    "random_scene": dict(camera="random", background="sky", max_depth=8),
    "cornell_box": dict(camera="final_alt", background="sky", max_depth=50),
    "final": dict(camera="final_alt", background="sky", max_depth=50),
}
SCENES = tuple(FRAMES)
BG = {"sky": rtnw.RT_BG_SKY, "black": rtnw.RT_BG_BLACK}

FAR = (N - T, 0, T, T)          # the top right corner: x at the limit, j = ny - 1 and below
CENTRE = (32764, 32763, T, T)   # holds (x, j) = (32768, 32768): the key crosses 2^31 inside it
# The same for a camera that looks level (final_alt: lookfrom.y = lookat.y = 278): image rows
# 32759..32766, so j = 32768..32775.  In image row 32767 of such a frame the primary rays'
# direction has y == 0 exactly (a pixel is 5.4e-5 high there and 278's ulp is 3.1e-5), and rays
# exactly parallel to an axis are not part of this parity contract (their rect hits divide by 0).
CENTRE_LEVEL = (32764, 32759, T, T)
CORNERS = ((0, 0, T, T), FAR, (0, N - T, T, T), (N - T, N - T, T, T))
PIXELS = ((0, 0, 1, 1), (N - 1, 0, 1, 1), (0, N - 1, 1, 1), (N - 1, N - 1, 1, 1))
# a row in the lower half and the column through the centre tile, 65535 = 8191 x 8 + 7 pixels
# each, a single band of one row and 8192 bands of one column
STRIPS = ((0, 45000, N, 1), (32768, 0, 1, N))


def centre(scene):
    return CENTRE if FRAMES[scene]["camera"] == "random" else CENTRE_LEVEL


def tiles(scene):
    return CORNERS + (centre(scene),)


def entry_tiles(scene):
    """Where every entry point is run: the far corner and the centre."""
    return (FAR, centre(scene))


@dataclass(frozen=True)
class Case:
    scene: str
    rect: tuple
    spp: int = 4
    chunk: int = 2
    seed: int = 3                # the smallest seed under which every case below is `powerful` (under 1 and 2
                                 # two pixels of one of final's far tiles are bit-equal)
    sample_offset: int = 0
    fold: bool = False           # RT_FLAG_RIGHT_FOLD against the oracle's right fold

    @property
    def name(self):
        x0, y0, w, h = self.rect
        s = f"{self.scene}-{x0}.{y0}.{w}x{h}-spp{self.spp}-chunk{self.chunk}-seed{self.seed:#x}"
        if self.sample_offset:
            s += f"-at{self.sample_offset:#x}"
        return s + ("-fold" if self.fold else "")

    @property
    def strip(self):
        return self.rect[2] * self.rect[3] > 4 * T * T

    def spec(self, **kw):
        """The oracle's statement of the case (oracle.kernel_spec), fields replaced by kw."""
        f = FRAMES[self.scene]
        a = dict(seed=self.seed, chunk=self.chunk, camera=f["camera"], background=f["background"],
                 max_depth=f["max_depth"], rect=self.rect, sample_offset=self.sample_offset)
        a.update(kw)
        ns = a.pop("ns", self.spp)
        s = O.kernel_spec(self.scene, N, N, ns, **a)
        s.forward = not self.fold
        return s

    def desc_spec(self, **kw):
        """The same for a descriptor render (oracle.first_hits_desc on the built-in's descriptor)."""
        f = FRAMES[self.scene]
        a = dict(seed=self.seed, chunk=self.chunk, background=f["background"], max_depth=f["max_depth"],
                 rect=self.rect, sample_offset=self.sample_offset)
        a.update(kw)
        return O.desc_spec(N, N, a.pop("ns", self.spp), **a)

    def params(self, **kw):
        """The rt_render_params of the case, fields replaced by kw."""
        f = FRAMES[self.scene]
        a = dict(max_depth=f["max_depth"], background=BG[f["background"]], chunk=self.chunk, seed=self.seed,
                 sample_offset=self.sample_offset, flags=rtnw.RT_FLAG_RIGHT_FOLD if self.fold else 0)
        a.update(kw)
        return rtnw.RenderParams(N, N, a.pop("spp", self.spp), **a)

    def camera(self):
        return rtnw.Camera.preset(FRAMES[self.scene]["camera"], N, N)


# 1. frames: every scene at every tile and corner pixel, and its two strips at 1 spp
FRAME_CASES = [Case(s, r) for s in SCENES for r in tiles(s) + PIXELS] + \
              [Case(s, r, spp=1, chunk=1) for s in SCENES for r in STRIPS]
# A strip's 65535 one-sample paths can hold rays exactly parallel to an axis: a diffuse bounce off
# a vertical wall at height p.y ~ 278 leaves with direction.y = (p.y + r.y) - p.y, which is 0
# whenever |r.y| is below half an ulp of p.y, about once in 10^4 paths of cornell_box.  Such rays
# are outside this parity contract; the pixels that hold one (oracle_image's mask) are left out
# of the strips' comparison, and there are exactly this many of them, none in any other case:
AXIS_PIXELS = {("cornell_box", STRIPS[0]): 10, ("cornell_box", STRIPS[1]): 13, ("final", STRIPS[0]): 3}
# (of cornell_box's 10 and 13, 7 and 11 differ on an MI355X; the others' paths go the same way)
# 2. every entry point at a far tile and at the centre (right fold; tiles in one call, moments,
#    adaptive and features are run on the plain cases of these tiles)
FOLD_CASES = [Case(s, r, chunk=1, fold=True) for s in SCENES for r in entry_tiles(s)]
ENTRY_CASES = [Case(s, r, chunk=1) for s in SCENES for r in entry_tiles(s)]
# the feature pass needs surfaces in view: the top right corner of random_scene's and of final's
# frame is sky, so their far tile is a bottom corner (x at the limit on random_scene and on
# cornell_box, y at the limit on random_scene and final)
FEATURE_FAR = {"random_scene": CORNERS[3], "cornell_box": FAR, "final": CORNERS[2]}
FEATURE_CASES = [Case(s, r, chunk=1) for s in SCENES for r in (FEATURE_FAR[s], centre(s))]
# 3. the last sample indices: spp 7 in chunks of 3 ending at index 0xFFFFFFFE
LAST_SPP = 7
LAST_CASES = [Case(s, FAR, spp=LAST_SPP, chunk=3, sample_offset=LAST - LAST_SPP, fold=fold)
              for s in SCENES for fold in (False, True)]
SUM_IN_CASES = [Case(s, FAR, spp=LAST_SPP, chunk=1, sample_offset=LAST - LAST_SPP) for s in ("cornell_box", "random_scene")]
# 4. chunks: INT_MAX with 3 samples, and spp + 1
CHUNK_CASES = [Case(s, FAR, spp=3, chunk=2 ** 31 - 1) for s in SCENES] + [Case(s, FAR, spp=3, chunk=4) for s in SCENES]
# 5. seeds, on one small frame (SEED_NX x SEED_NY, the whole of it)
SEEDS = (0, 1 << 63, 2 ** 64 - 1)
SEED_SCENE, SEED_NX, SEED_NY, SEED_SPP = "random_scene", 24, 16, 4

# every case whose oracle image a GPU test compares with
POWER_CASES = FRAME_CASES + FOLD_CASES + ENTRY_CASES + LAST_CASES + SUM_IN_CASES + CHUNK_CASES

# the adaptive renders at the entry tiles: (min_spp, step_spp, cap), tolerance, floor
# (on the oracle's samples of cornell_box both tiles stop at four counts without a guard and at
# two or three with radius 2: test_limits_spec.py)
ADAPTIVE = dict(mn=2, step=2, cap=8, tol=0.8, floor=0.01)
ADAPTIVE_SCENE = "cornell_box"


def seed_spec(seed, **kw):
    f = FRAMES[SEED_SCENE]
    return O.kernel_spec(SEED_SCENE, SEED_NX, SEED_NY, SEED_SPP, seed=seed, chunk=2, camera=f["camera"],
                         background=f["background"], max_depth=f["max_depth"], **kw)


def pixel_bits(img):
    """[npix, 3] uint32: every pixel's three floats as bits."""
    return np.ascontiguousarray(img, np.float32).view(np.uint32).reshape(-1, 3)


def power(img):
    """(share of nonzero pixels, nonzero pixels that bit-equal an earlier one, share of the
    pixels that are nonzero and bitwise unique in the image)."""
    px = pixel_bits(img)
    nz = px[(px != 0).any(axis=1)]
    _, counts = np.unique(nz, axis=0, return_counts=True)
    return len(nz) / len(px), int(len(nz) - len(counts)), float((counts == 1).sum()) / len(px)


def powerful(img):
    share, equal, _ = power(img)
    return share >= 0.5 and equal == 0


def powerful_strip(img):
    return power(img)[2] >= 0.5




def oracle_image(case, threads=1, **kw):
    """(image, axis mask) of the case in the oracle's statement, fields replaced by kw: the mask
    [h, w] marks the pixels one of whose rays, at any bounce, had a direction component of
    exactly 0 (oracle.render's `axis`).  Such rays are outside the parity contract (a rect's hit
    divides by the component), and the mask is what a comparison leaves out."""
    spec = case.spec(threads=threads, **kw)
    mask = np.zeros((spec.rect[3], spec.rect[2]), np.uint8)
    img = O.render(spec, axis=mask)[0]
    return img, mask.astype(bool)
