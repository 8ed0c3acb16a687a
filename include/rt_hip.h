/* include/rt_hip.h — C ABI of librt_hip.so, the MI355X path tracer.
 *
 * Boundary being replaced (the reference has no FFI; its hot path is a C++ call
 * pair):
 *   vec3 color(const ray&, hitable *world, int depth)      main.cpp:25-46
 *   the per-pixel sample loop of main()                     main.cpp:299-332
 *   hitable::hit / material::scatter / texture::value       hitable.h:34, material.h:54, texture.h:13
 * The host keeps the reference's hitable/material/texture/camera classes (see
 * peter-shirley-ray-tracing-the-next-week_amd/csrc/host/rtnw.h); a world built
 * with them is flattened into an rt_scene_desc, uploaded once with
 * rt_scene_create, and rendered on the GPU with rt_render_tile / rt_render_tiles.
 *
 * Conventions: plain C types only; every function returns RT_OK (0) or a
 * negative rt_status; rt_last_error() returns a thread-local message.  A scene is
 * bound to one HIP device; calls on one scene are serialised on a stream.  There
 * is no CPU fallback: without a usable GPU every render entry point fails.
 */
#ifndef RT_HIP_H
#define RT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: rt_stats gained the shading-stage divergence fields (wave_shade_passes ...) */
#define RT_ABI_VERSION 2

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,      /* bad argument / malformed descriptor */
    RT_ERR_HIP = -2,          /* HIP runtime failure (no device, launch error, ...) */
    RT_ERR_NOMEM = -3,
    RT_ERR_UNSUPPORTED = -4   /* a scene feature the device path does not implement */
} rt_status;

/* ------------------------------------------------------------ scene descriptor
 * Flattened form of a hitable tree.  Leaves are listed in depth-first list order
 * (the order hitable_list::hit visits them, hitable_list.h:24); that order is the
 * tie-break order of the closest-hit search.                                   */
enum rt_prim_kind {
    RT_PRIM_SPHERE = 0,          /* sphere.h:10-52:  p = {cx, cy, cz, r}                      */
    RT_PRIM_MOVING_SPHERE = 1,   /* sphere.h:61-118: p = {c0x,c0y,c0z, c1x,c1y,c1z, t0, t1, r} */
    RT_PRIM_XY_RECT = 2,         /* aarect.h:11-65:  p = {x0, x1, y0, y1, k}                  */
    RT_PRIM_XZ_RECT = 3,         /* aarect.h:23-83:  p = {x0, x1, z0, z1, k}                  */
    RT_PRIM_YZ_RECT = 4          /* aarect.h:35-100: p = {y0, y1, z0, z1, k}                  */
};

typedef struct rt_prim {
    int32_t kind;        /* rt_prim_kind */
    int32_t material;    /* index into rt_scene_desc.materials */
    int32_t instance;    /* -1, or index into rt_scene_desc.instances (transform chain) */
    int32_t flip;        /* 1: a flip_normals wraps the primitive directly (hitable.h:39-54) */
    float p[12];
} rt_prim;               /* 64 bytes */

enum rt_xform_op {
    RT_OP_TRANSLATE = 1, /* hitable.h:57-83:  {ox, oy, oz}            */
    RT_OP_ROTATE_Y = 2,  /* hitable.h:85-150: {sin_theta, cos_theta}  */
    RT_OP_FLIP = 3       /* hitable.h:39-54 between two transforms    */
};

typedef struct rt_instance {
    int32_t nops;        /* <= 6; ops[0] is the outermost wrapper */
    int32_t pad[3];
    float ops[6][4];     /* {op, a, b, c} */
} rt_instance;

enum rt_material_kind {
    RT_MAT_LAMBERTIAN = 0,    /* material.h:61-72   texture        */
    RT_MAT_METAL = 1,         /* material.h:74-85   albedo, fuzz   */
    RT_MAT_DIELECTRIC = 2,    /* material.h:87-123  ref_idx        */
    RT_MAT_DIFFUSE_LIGHT = 3, /* material.h:126-139 texture        */
    RT_MAT_ISOTROPIC = 4      /* material.h:142-151 texture        */
};

typedef struct rt_material {
    int32_t kind;
    int32_t texture;     /* -1 when unused */
    float fuzz;          /* already clamped to <= 1 (material.h:76) */
    float ref_idx;
    float albedo[3];
    int32_t pad;
} rt_material;           /* 32 bytes */

enum rt_texture_kind {
    RT_TEX_CONSTANT = 0, /* texture.h:16-27 color                    */
    RT_TEX_CHECKER = 1,  /* texture.h:30-45 even, odd (texture idx)  */
    RT_TEX_NOISE = 2,    /* texture.h:48-59 scale                    */
    RT_TEX_IMAGE = 3     /* surface_texture.h:10-30 image (index into images)      */
};

typedef struct rt_texture {
    int32_t kind;
    int32_t even, odd;   /* checker children */
    float scale;         /* noise */
    float color[3];      /* constant */
    int32_t image;       /* image: index into rt_scene_desc.images */
} rt_texture;            /* 32 bytes */

typedef struct rt_image {    /* texels of one image_texture (surface_texture.h:13) */
    int64_t offset;          /* byte offset into rt_scene_desc.image_data */
    int32_t nx, ny;          /* image size; texel (i, j) channel c is at 3*i + 3*nx*j + c
                                (surface_texture.h:26-28 addresses with stride 3 whatever
                                the file's channel count) */
} rt_image;

typedef struct rt_medium {   /* constant_medium.h:14-50 */
    int32_t boundary_first;  /* range in rt_scene_desc.boundary_prims */
    int32_t boundary_count;  /* >= 1: a medium needs at least one boundary primitive
                                (rt_scene_create returns RT_ERR_UNSUPPORTED for 0) */
    float density;
    int32_t material;        /* the isotropic phase material */
    int32_t order;           /* number of surface prims before it in list order */
    int32_t pad[3];
} rt_medium;

typedef struct rt_scene_desc {
    uint32_t abi_version;         /* RT_ABI_VERSION */
    int32_t nprims, nboundary, nmedia, nmaterials, ntextures, ninstances;
    const rt_prim *prims;         /* surfaces, depth-first list order */
    const rt_prim *boundary_prims;/* leaves of media boundaries */
    const rt_medium *media;       /* in list order (= keyed-draw ordinal) */
    const rt_material *materials;
    const rt_texture *textures;
    const rt_instance *instances;
    const float *perlin_ranvec;   /* 256 x 3, perlin.h:82-87 */
    const int32_t *perlin_perm;   /* 3 x 256, perlin.h:99-111 */
    float time0, time1;           /* shutter span rays may carry (moving-sphere bounds) */
    int32_t nimages;
    const rt_image *images;
    const uint8_t *image_data;    /* texel bytes of all images */
    int64_t image_bytes;
} rt_scene_desc;

/* ------------------------------------------------------------------ camera */
typedef struct rt_camera_desc {   /* the state camera.h:21-39 computes */
    float origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];
    float lens_radius, time0, time1;
} rt_camera_desc;

/* Same arithmetic as camera::camera (camera.h:21-39). */
int rt_camera_init(rt_camera_desc *out, const float lookfrom[3], const float lookat[3], const float vup[3],
                   float vfov, float aspect, float aperture, float focus_dist, float t0, float t1);

/* ------------------------------------------------------------------ render */
enum { RT_BG_BLACK = 0, RT_BG_SKY = 1 };
enum {
    RT_FLAG_COUNT = 1,            /* counting variant: fills the rt_stats visit counters */
    RT_FLAG_PROFILE = 2,          /* stamp variant: fills cycles_* (diagnostic; never timed) */
    /* Progressive rendering / checkpoint-resume: the output holds per-pixel
     * SUMS instead of means.  SUM_IN: on entry the output already holds the sums of
     * samples [0, sample_offset) (e.g. read back from rt_checkpoint_read); this call
     * adds samples [sample_offset, sample_offset + spp) to them one at a time, in
     * sample order, so a resumed render is bitwise the uninterrupted one.  SUM_OUT:
     * write the sums (to checkpoint or resume later); without it the output is the
     * mean, col * float(1.0 / ns) with ns = sample_offset + spp under SUM_IN, else spp. */
    RT_FLAG_SUM_IN = 4,
    RT_FLAG_SUM_OUT = 8,
    /* Parity mode (DESIGN.md §7 "Right-fold mode"; speed is not its goal): each sample's
     * radiance is computed as main.cpp:36's `emitted + attenuation*color(...)` from the
     * deepest hit outwards (a right fold over the path's scatters), not by forward
     * throughput.  The image then equals the reference binary's counter-RNG framebuffer
     * bit for bit when chunk <= 1 or chunk >= spp (one add per sample, main.cpp:311).
     * Media are still evaluated after the surface pass, not in list order (the DESIGN
     * section records why no input tells the two apart).  Composes with sample_offset,
     * SUM_IN / SUM_OUT, chunk, tiles and sample batches like a plain render; with
     * RT_FLAG_COUNT or RT_FLAG_PROFILE it returns RT_ERR_INVALID, on a scene with a wide
     * BVH (RTNW_BVH_WIDTH 4, 8, 8q) RT_ERR_UNSUPPORTED.  Every lane of the launch keeps a
     * stack of max_depth attenuations (16 B each) in device memory; a max_depth whose
     * stacks would pass the slab budget's default (16 GiB) returns RT_ERR_INVALID. */
    RT_FLAG_RIGHT_FOLD = 16
};

/* Limits, checked by every render entry point with its other arguments (RT_ERR_INVALID, the
 * output untouched):
 *   nx, ny          1..65535 each.  A tile may lie anywhere inside the frame; the pixel key of
 *                   (x, j) is the uint32_t j * nx + x, below 2^32 for every such frame.
 *   sample range    spp >= 1 and (uint64_t)sample_offset + spp <= 0xFFFFFFFF: sample indices
 *                   are 32-bit, and the count sample_offset + spp, the mean's divisor under
 *                   RT_FLAG_SUM_IN, is a uint32_t too.
 *   chunk           any positive int32 (larger than spp: one work item per pixel); <= 0 selects 1.
 *   seed            any uint64_t. */
typedef struct rt_render_params {
    int32_t nx, ny;               /* full image (u,v normalisation and pixel keys), 1..65535 each */
    int32_t spp;                  /* samples per pixel (main.cpp:251 ns) */
    int32_t max_depth;            /* scatter while depth < max_depth (main.cpp:34: 50) */
    float t_min;                  /* main.cpp:27: 0.001 */
    int32_t background;           /* RT_BG_* */
    int32_t chunk;                /* samples per work item (partial sum); <= 0 selects 1, the
                                     reference's one-add-per-sample order (main.cpp:311).  A job
                                     whose partial-sum slab (16 B x pixels x ceil(spp/chunk))
                                     would pass the slab budget (8 GiB, env RTNW_SLAB_BUDGET) runs
                                     as several launches over sample batches, each batch added
                                     to a per-pixel running sum in sample order: the image does
                                     not depend on the job's size or split (any rank count) */
    int32_t flags;                /* RT_FLAG_* */
    uint32_t sample_offset;       /* first sample index (progressive rendering); sample_offset + spp <= 0xFFFFFFFF */
    uint32_t pad;
    uint64_t seed;                /* counter-RNG key */
} rt_render_params;

typedef struct rt_stats {
    double samples;               /* camera samples rendered */
    double segments;              /* rays traced = world hit calls (RT_FLAG_COUNT) */
    double node_visits;           /* BVH2 nodes fetched, each holding both child boxes (RT_FLAG_COUNT) */
    double sphere_tests;          /* sphere tests, BVH leaves + media boundaries (RT_FLAG_COUNT) */
    double moving_sphere_tests;   /* (RT_FLAG_COUNT) */
    double rect_tests;            /* xy/xz/yz rect tests (RT_FLAG_COUNT) */
    double instanced_tests;       /* tests through a translate/rotate_y chain (RT_FLAG_COUNT) */
    double medium_tests;          /* constant_medium evaluations (RT_FLAG_COUNT) */
    double shades;                /* material evaluations (RT_FLAG_COUNT) */
    double noise_evals;           /* Perlin turbulence evaluations (RT_FLAG_COUNT) */
    double algorithmic_bytes;     /* SURVEY §8d byte model for the launch (RT_FLAG_COUNT) */
    double kernel_ms;             /* megakernel time from HIP events on the render stream */
    double resolve_ms;            /* partial-sum resolve kernel time */
    double cycles_claim;          /* RT_FLAG_PROFILE: wave cycles in work claim + camera sampling */
    double cycles_traverse;       /*   ... in the BVH / primitive search */
    double cycles_media;          /*   ... in constant_medium evaluation + hit record */
    double cycles_shade;          /*   ... in material / texture evaluation */
    double grid;                  /* workgroups launched (persistent grid) */
    double wave_iterations;       /* RT_FLAG_COUNT: megakernel loop iterations, summed over waves */
    double wave_node_trips;       /*   wave-level BVH node steps (SIMD efficiency = node_visits / 64x this) */
    double wave_prim_trips;       /*   wave-level primitive-test steps */
    double wave_sphere_draw_trips;/*   wave-level random_in_unit_sphere rejection rounds */
    double lane_sphere_draw_trips;/*   lane-level rejection rounds */
    double chunk;                 /* samples per work item the launch used (rt_render_params.chunk or its default) */
    double batches;               /* megakernel launches (sample batches) the job took */
    double lds_level;             /* scene data in LDS: 0 none (HBM, L1/L2), 1 the BVH2 nodes */
    double stack_depth;           /* traversal stack entries per lane (LDS variants: the BVH depth + 1) */
    double scan_groups;           /* flat scan instead of a BVH (<= 64 primitives): its instance groups, else 0 */
    double prescan;               /* BVH scenes: largest primitives kept out of the BVH, tested first in lockstep */
    double wave_exhaust_first_us; /* RT_FLAG_PROFILE wave timeline of the job's last launch (s_memrealtime, us
                                     after its first wave started):
                                     the first wave to find the work pool empty */
    double wave_exhaust_last_us;  /*   the last wave to find it empty */
    double wave_end_first_us;     /*   the first wave to finish */
    double wave_end_mean_us;      /*   mean wave finish */
    double wave_end_last_us;      /*   the last wave to finish (the launch's end) */
    double wave_shade_passes;     /* RT_FLAG_COUNT: wave-level passes through the material scatter branches */
    double wave_shade_kinds;      /*   distinct scatter materials (lambertian/metal/dielectric/isotropic) summed
                                         over those passes: the branches each pass ran */
    double lane_scatters;         /*   lanes that scattered (SIMD efficiency = this / 64x wave_shade_passes) */
    double cycles_scatter;        /* RT_FLAG_PROFILE: wave cycles in the material scatter branches (part of
                                         cycles_shade) */
    double ball_fused_scatters;   /* RT_FLAG_COUNT: lanes served by the ball waves' fused in-ball step, that is
                                         segments that scattered at a medium there (part of lane_scatters) */
    double ball_fused_declined;   /*   eligible lanes a trip of that step left to the generic stages (a cell
                                         primitive first, the cell undecided, or no scatter); both are 0 in a
                                         kernel variant without ball waves */
    double empty_fast_samples;    /* RT_FLAG_COUNT: camera samples of provably empty pixels that the work claim
                                         finished itself (no surface in reach, no medium scattered): counted in
                                         samples and segments, never seen by the traversal; 0 with
                                         RTNW_EMPTY_FAST=0 or in a render that leaves the feature off */
    double empty_pixels;          /* job pixels flagged as provably empty for this render (0: feature off) */
} rt_stats;

typedef struct rt_scene rt_scene; /* opaque; owns device copies */

/* Copies the descriptor into device memory (HBM) of `device` and builds the BVH.
 * The caller keeps ownership of d. */
int rt_scene_create(const rt_scene_desc *d, int device, rt_scene **out);
void rt_scene_destroy(rt_scene *s);

/* Renders the w x h rectangle at (x0, y0) (image coords, row 0 = top row of the
 * PPM, i.e. main.cpp's j = ny-1) into out_rgb (host memory, h*w*3 floats, linear
 * mean radiance = main.cpp's `col` after `col /= float(ns)`).  Synchronous. */
int rt_render_tile(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                   int x0, int y0, int w, int h, float *out_rgb, rt_stats *stats);

/* Renders ntiles rectangles (tiles[4k..4k+3] = x0, y0, w, h) into device memory:
 * out_dev receives the tiles packed back to back (tile k at offset sum_{i<k} w_i*h_i*3
 * floats, each row-major).  Enqueued on `stream` (a hipStream_t; NULL = default
 * stream).  When stats is non-NULL the call waits for completion to read the
 * HIP-event timings.  ntiles == 0 is a no-op (a rank without tiles). */
int rt_render_tiles(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                    const int32_t *tiles, int ntiles, float *out_dev, void *stream, rt_stats *stats);

/* Device buffer helpers, so callers without a HIP toolchain can drive the ABI. */
int rt_device_alloc(int device, uint64_t bytes, void **out);
int rt_device_free(void *ptr);
int rt_copy_to_host(void *dst, const void *src_dev, uint64_t bytes);
int rt_copy_to_device(void *dst_dev, const void *src, uint64_t bytes);
int rt_device_count(int *out);

/* ------------------------------------------- moments and adaptive sampling */
/* rt_render_tiles + per-pixel moments of the work items' channel sums y = (r+g)+b:
 * moments_dev receives 2 floats per pixel (sum y, sum y*y; float32, item order) in the packed
 * tile layout.  With RT_FLAG_SUM_IN both out_dev and moments_dev hold the earlier samples'
 * values on entry.  out_dev is bitwise what rt_render_tiles writes.  The moments are sums
 * whatever RT_FLAG_SUM_OUT says, and do not depend on the sample batches.  With RT_FLAG_COUNT
 * or RT_FLAG_PROFILE it returns RT_ERR_INVALID. */
int rt_render_tiles_moments(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                            const int32_t *tiles, int ntiles, float *out_dev, float *moments_dev,
                            void *stream, rt_stats *stats);

typedef struct rt_adaptive_params {
    int32_t min_spp;    /* first pass, every pixel; >= 2 */
    int32_t step_spp;   /* samples each later pass adds to the pixels still active; >= 1;
                           the last pass is clipped so that no pixel passes p->spp */
    float tolerance;    /* relative standard error; <= 0: no pixel ever converges */
    float floor;        /* >= 0, added to the mean of y: dark pixels converge too */
} rt_adaptive_params;

typedef struct rt_adaptive_stats {
    double passes;            /* megakernel passes (the first over every pixel) */
    double samples;           /* camera samples rendered = the sum of out_spp */
    double pixels_converged;  /* pixels the rule stopped, those it stopped at the cap included */
    double pixels_capped;     /* pixels still active after p->spp samples */
    double kernel_ms, resolve_ms, select_ms;   /* HIP-event times summed over the passes */
} rt_adaptive_stats;

/* Error-driven render of the w x h rectangle at (x0, y0): every pixel gets min_spp samples,
 * then step_spp more per pass while it is active, up to p->spp (the cap).  With one sample
 * per work item (chunk is forced to 1), y = (r+g)+b of a sample, n the pixel's samples so
 * far, S1 = sum y and S2 = sum y*y (float32 sums in sample order, read as doubles), a pixel
 * leaves the active set for good after a pass when, in FP64 and in exactly this order,
 *     N*S2 - S1*S1  <=  ((tol*tol) * (N - 1.0)) * (t*t),   t = S1 + floor*N
 * i.e. the standard error of the mean of y <= tolerance x (mean of y + floor), with the N-1
 * sample variance; a NaN moment compares false, and tolerance <= 0 skips the comparison: no
 * pixel converges.  A pixel that received n samples is bitwise that pixel of
 * rt_render_tile(spp = n): out_rgb holds sum * float(1.0 / n) with the pixel's own n.
 * p->spp is the cap.  out_rgb: h*w*3 host floats (mean); out_spp: h*w int32 (may be NULL);
 * out_moments: h*w*2 floats (may be NULL); stats may be NULL.  Synchronous.
 * RT_ERR_INVALID for a null argument, min_spp < 2, step_spp < 1, p->spp < min_spp, a negative
 * or non-finite floor, a NaN tolerance, p->sample_offset != 0 or any of RT_FLAG_COUNT,
 * RT_FLAG_PROFILE, RT_FLAG_SUM_IN, RT_FLAG_SUM_OUT; RT_FLAG_RIGHT_FOLD passes through. */
int rt_render_adaptive(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                       const rt_adaptive_params *ap, int x0, int y0, int w, int h,
                       float *out_rgb, int32_t *out_spp, float *out_moments, rt_adaptive_stats *stats);

/* rt_render_adaptive with a neighbourhood guard on the stop rule: same
 * arguments, checks and outputs, plus guard_radius r in 0..8 (otherwise RT_ERR_INVALID, checked
 * with the other arguments before the device is touched).  After each pass's samples every
 * active pixel takes the test above unchanged; fail(q) = q is active and its test fails (a
 * retired pixel never fails: its moments are frozen and it passed on them).  An active pixel
 * p leaves the active set iff no pixel q of the rendered rectangle with |qx - px| <= r and
 * |qy - py| <= r has fail(q): the window is clipped to the w x h rectangle, nothing outside it
 * exists.  A retired pixel never returns, and at the cap every active pixel stops.  So:
 *   - r = 0 is rt_render_adaptive bit for bit: image, counts, moments and the stats' passes,
 *     samples, pixels_converged and pixels_capped;
 *   - a pixel that received n samples is still bitwise that pixel of rt_render_tile(spp = n);
 *   - every pixel's count is >= its count under rt_render_adaptive with the same parameters:
 *     a pixel can only retire after a pass at which its own test passes;
 *   - tolerance <= 0 is still the fixed render at the cap;
 *   - a tile is NOT the crop of the frame's result (it is for rt_render_adaptive), since the
 *     window sees only the rectangle rendered.
 * pixels_converged counts the pixels that retired, those that retired after the last pass
 * included; pixels_capped those a failing neighbour (or their own test) still held then. */
int rt_render_adaptive_guarded(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                               const rt_adaptive_params *ap, int guard_radius, int x0, int y0, int w, int h,
                               float *out_rgb, int32_t *out_spp, float *out_moments, rt_adaptive_stats *stats);

/* ------------------------------- first-hit features and the denoiser */
/* Feature buffers of the w x h rectangle at (x0, y0): per pixel the mean, over samples
 * [sample_offset, sample_offset + spp), of each sample's first surface hit.  Sample k of a
 * pixel is the camera ray rt_render_tile traces for that sample (same key, jitter, lens and
 * time draws), and its hit the closest one under the (t, list order) rule:
 *   albedo   (3)  the hit material's colour: the texture's value at the hit for a lambertian,
 *                 a diffuse light and an isotropic material, the albedo of a metal, (1, 1, 1)
 *                 for a dielectric; (1, 1, 1) on a miss
 *   normal   (3)  the hit record's normal in world space (flip_normals, negative radii and
 *                 instance chains applied; not normalised again); (0, 0, 0) on a miss
 *   depth    (1)  t * |direction|; 0 on a miss
 *   coverage (1)  1 on a hit, 0 on a miss
 * The samples are added in sample order in float32 and the sum is multiplied by
 * float(1.0 / spp), as rt_render_tile does with the radiance.  Constant media are ignored: the
 * features see through them to the surface behind.  Used from p: nx, ny, spp, sample_offset,
 * seed, t_min; max_depth, background, chunk and RT_FLAG_RIGHT_FOLD are ignored.
 * RT_ERR_INVALID for a null argument, all four outputs null, nx or ny < 1, spp < 1, a
 * rectangle outside the image and any of RT_FLAG_COUNT, RT_FLAG_PROFILE, RT_FLAG_SUM_IN,
 * RT_FLAG_SUM_OUT (all checked before the device is touched); RT_ERR_UNSUPPORTED on a scene
 * with a wide BVH (RTNW_BVH_WIDTH 4, 8, 8q).
 * Host buffers (any of the four may be NULL, not all), row-major h x w.  Synchronous. */
int rt_render_features(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                       int x0, int y0, int w, int h,
                       float *albedo, float *normal, float *depth, float *coverage);
/* The same into device memory, enqueued on `stream` (hipStream_t, NULL = default): 8 floats
 * per pixel, (albedo.rgb, coverage, normal.xyz, depth), row-major h x w — the guides
 * rt_denoise_dev reads. */
int rt_render_features_dev(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                           int x0, int y0, int w, int h, float *guides_dev, void *stream);

typedef struct rt_denoise_params {
    int32_t iterations;
    int32_t demodulate;
    float sigma_color, sigma_depth;
    int32_t uniform_spp;
    int32_t variance_filter;
    int32_t pad[2];
} rt_denoise_params;
/* rt_denoise_params: iterations 0..8 (0 copies the input); demodulate 0 / 1: filter
 * colour / max(albedo, 0.01) and multiply the albedo back afterwards; sigma_color, sigma_depth
 * >= 0 (suggested: 2, 1, with 3 iterations and demodulation); uniform_spp: the
 * sample count of every pixel when no per-pixel map is given; variance_filter 0 / 1 (any other
 * value is RT_ERR_INVALID; it took the place of a pad word, so a zeroed struct keeps the
 * filter of before bit for bit): with 1 and moments present, the luminance weight of every
 * iteration measures the difference against the 3 x 3 Gaussian (1 2 1 / 4 each way, the direct
 * neighbours, the centre in place of a neighbour outside the image) of that iteration's input
 * variance instead of the centre pixel's own (Schied et al. 2017); the variance propagated to
 * the next iteration is still the unfiltered one's.  Without moments it has no effect.  The
 * exact statement is tests/test_denoise_varfilter_spec.py. */

/* Edge-avoiding à-trous wavelet filter (5 x 5 B3-spline taps, 2^i pixels apart in iteration i)
 * of an nx x ny image.  A tap's weight is the spline's times three edge-stopping terms: the
 * normals' dot product to the power 128, the relative depth difference (sigma_depth), and —
 * when moments are given — the luminance difference against the centre pixel's standard error
 * (sigma_color), from the moments rt_render_tiles_moments / rt_render_adaptive write and each
 * pixel's sample count (spp map, or uniform_spp when spp is NULL); the variance is filtered
 * along.  The exact float32 statement is tests/test_denoise_spec.py.  Depths must not be
 * negative.  Host buffers: color nx*ny*3; albedo, normal, depth as rt_render_features writes
 * them; moments nx*ny*2 or NULL; spp nx*ny or NULL; out nx*ny*3; *ms (when non-NULL) receives
 * the kernels' time in ms.  Synchronous.
 * RT_ERR_INVALID for a null pointer, nx or ny < 1, iterations outside 0..8, a negative or NaN
 * sigma, uniform_spp < 1 with moments and no spp map, and a variance_filter other than 0 or 1
 * (checked before the device is touched). */
int rt_denoise(int device, int nx, int ny, const float *color, const float *albedo, const float *normal,
               const float *depth, const float *moments, const int32_t *spp, const rt_denoise_params *dp,
               float *out, double *ms);
/* The same on device buffers, enqueued on `stream`: color_dev 3 floats per pixel (as
 * rt_render_tiles packs one full-frame tile), guides_dev from rt_render_features_dev,
 * moments_dev and spp_dev may be NULL.  The filter's planes live in a per-device workspace
 * that grows on demand: calls on one device must not overlap. */
int rt_denoise_dev(int device, int nx, int ny, const float *color_dev, const float *guides_dev,
                   const float *moments_dev, const int32_t *spp_dev, const rt_denoise_params *dp,
                   float *out_dev, void *stream);

/* ------------------------------- firefly clamp ahead of the denoiser */
typedef struct rt_firefly_params {       /* 32 bytes */
    int32_t demodulate;    /* 0 / 1 */
    int32_t radius;        /* 1..3 */
    int32_t min_similar;   /* 1..(2r+1)^2 - 1 */
    float k;               /* >= 1 */
    float floor;           /* >= 0, finite */
    float cos_normal;      /* -1..1 */
    float sigma_depth;     /* >= 0 */
    float sigma_albedo;    /* >= 0 */
} rt_firefly_params;
/* Guide-aware outlier clamp of an nx x ny image, one Jacobi pass (every value read is an
 * input).  With a' = max(albedo, 0.01) per channel when demodulate, else 1, a pixel's
 * luminance is l = the sum of colour / a' over the channels.  A neighbour q within `radius`
 * of p (a (2r+1)^2 window without its centre; neighbours outside the image do not exist) is
 * similar when n_p . n_q >= cos_normal, |z_p - z_q| <= sigma_depth * min(z_p, z_q) + 1e-6 and
 * |s_p - s_q| <= sigma_albedo * min(s_p, s_q) + 1e-6, s the sum of the raw albedo's channels.
 * A pixel with at least min_similar similar neighbours whose l exceeds
 * bound = k * (their mean l) + floor is scaled by ratio = bound / l: colour, and the moments
 * as if every sample of the pixel had been scaled (m1 * ratio, m2 * ratio^2), so they feed
 * rt_denoise as they are.  Every other pixel is copied bit for bit (ratio 1).  A one-pixel
 * light keeps its value: its guide albedo is its emission, no neighbour resembles it, and it
 * stays below min_similar.  Misses (normal 0, depth 0) resemble each other only when
 * cos_normal <= 0.  The exact float32 statement is tests/test_firefly_spec.py.  Inputs must be
 * finite and depths non-negative.  Suggested: demodulate 1, radius 2, min_similar 3, k 8,
 * floor 0.01, cos_normal 0.9, sigma_depth 0.1, sigma_albedo 0.25 (what the
 * clamp buys, and that it never lowers the error against a reference).
 * Host buffers: color nx*ny*3; albedo, normal, depth as rt_render_features writes them;
 * moments nx*ny*2 or NULL; out nx*ny*3, not color (neighbours are read: the pass cannot run
 * in place); out_moments nx*ny*2 or NULL, needs moments and may be moments itself; ratio nx*ny
 * or NULL; *ms (when non-NULL) receives the kernel's time in ms.  Synchronous.
 * RT_ERR_INVALID for a null required pointer, nx or ny < 1 or nx * ny >= 2^31, a parameter
 * outside the ranges above or NaN, out_moments without moments, and out == color (all checked
 * before the device is touched, the parameter named in rt_last_error()). */
int rt_firefly(int device, int nx, int ny, const float *color, const float *albedo, const float *normal,
               const float *depth, const float *moments, const rt_firefly_params *fp,
               float *out, float *out_moments, float *ratio, double *ms);
/* The same on device buffers, enqueued on `stream`: color_dev 3 floats per pixel, guides_dev
 * from rt_render_features_dev; moments_dev, out_moments_dev and ratio_dev may be NULL.  No
 * workspace: calls may overlap. */
int rt_firefly_dev(int device, int nx, int ny, const float *color_dev, const float *guides_dev,
                   const float *moments_dev, const rt_firefly_params *fp, float *out_dev,
                   float *out_moments_dev, float *ratio_dev, void *stream);

/* ------------------------------- reprojected frame history ahead of the denoiser */
typedef struct rt_temporal_frame {   /* one struct for the frame, the history and the output */
    const float   *color;    /* nx*ny*3, mean radiance */
    const float   *guides;   /* nx*ny*8 as rt_render_features_dev packs them:
                                albedo.rgb, coverage, normal.xyz, depth */
    const float   *moments;  /* nx*ny*2 (sum y, sum y*y) or NULL */
    const int32_t *len;      /* nx*ny samples those sums and that mean stand for;
                                NULL in the current frame (every pixel: frame_spp) */
} rt_temporal_frame;
typedef struct rt_temporal_params {      /* 32 bytes */
    int32_t max_history;   /* 0..2^23 samples of history a pixel may carry */
    float cos_normal;      /* -1..1 */
    float sigma_depth;     /* >= 0 */
    int32_t frame_spp;     /* 1..65535: the samples behind every pixel of the current frame */
    int32_t pad[4];        /* zero */
} rt_temporal_params;
/* Temporal accumulation (Schied et al. 2017, the step ahead of the filter): blends the current
 * frame into the previous call's output, fetched where each pixel's surface point was seen by
 * the previous camera.  One Jacobi pass (every value read is an input) over nx x ny pixels, row
 * 0 on top.  `cur` is the frame (colour and moments as rt_render_tiles_moments writes them,
 * guides as rt_render_features_dev does, len NULL), `hist` the previous call's `out` with the
 * guides of that call's `cur`, or NULL for a first frame; `out` receives colour, moments (when
 * given) and len — what rt_denoise reads as color, moments and spp.  out->guides is ignored and
 * the pointers of `out` are written through: the caller keeps cur->guides as the next call's
 * hist->guides.  With n_f = frame_spp:
 *   No history (a first frame; or, below, W = 0, coverage != 1 under unequal cameras, n_h <= 0):
 *     the output pixel is the frame's bit for bit, the moments the frame's, len = n_f.
 *   Equal cameras (the two rt_camera_desc bytewise equal): a pixel's history is its own pixel
 *     of `hist`, weight 1, no tests — the scene cannot change between calls, so nothing is
 *     disoccluded; misses accumulate too.  n_h = min(hist len, max_history).
 *   Otherwise a pixel (x, y) with coverage exactly 1 is reprojected: P = origin + dir *
 *     (depth / |dir|), dir the camera's ray through the pixel centre and the lens centre,
 *     s = (x + 0.5) / nx, t = ((ny - 1 - y) + 0.5) / ny.  With d = P - origin', P must lie in
 *     front of the previous camera (d . w' < 0); d meets the plane of lower_left_corner',
 *     horizontal', vertical' at (s', t'), read by projection on horizontal' and vertical';
 *     fx = s' nx - 0.5, fy = (ny - 1) - (t' ny - 0.5), and the expected depth is z' = |d|.  Of the
 *     four bilinear taps around (fx, fy) a tap q counts when its weight is positive, it is inside
 *     the image, hist len[q] > 0, its coverage is exactly 1, n_p . n_q >= cos_normal and
 *     |z' - z_q| <= sigma_depth * min(z', z_q) + 1e-6 (rt_firefly's depth test).  W is the sum of
 *     the counting taps' weights; the history colour and per-sample moments mu = M / len are
 *     their weight-normalised sums, n_h = min(min of their len, max_history).
 *   Blend, n = n_h + n_f, a = float(n_f) / float(n): out = c_h + (c_f - c_h) * a, the same for
 *     mu_1 and mu_2 against the frame's S / n_f; out moments = (mu_1 n, mu_2 n), out len = n: a
 *     running mean until max_history, an exponential one after it, and an honest count.
 * The exact float32 statement is tests/test_temporal_spec.py.  Inputs must be finite and depths
 * non-negative.  Every call must be given a fresh sample range — sample_offset advanced by
 * frame_spp from frame to frame: equal ranges at an equal camera repeat the same samples, and
 * the accumulated count then claims samples that were never drawn.  Suggested: cos_normal 0.9,
 * sigma_depth 0.1 (rt_firefly's), max_history 16 (DESIGN.md §7h records the sweep: beyond it
 * the resampled history of a moving camera drifts faster than its noise falls).
 * Host form: host pointers in all three frames; one staging allocation; *ms (when non-NULL)
 * receives the kernel's time in ms.  Synchronous.
 * RT_ERR_INVALID — all checked before the device is touched, the parameter named in
 * rt_last_error() — for a null cur, cam, tp or out, a null cur->color, cur->guides, out->color
 * or out->len, with a history a null prev_cam, hist->color, hist->guides or hist->len; nx or
 * ny < 1 or nx * ny >= 2^31; a parameter outside the ranges above, NaN, or a nonzero pad;
 * cur->moments and hist->moments not both given or both NULL, out->moments given without
 * cur->moments; out->color equal to cur->color or hist->color, out->moments equal to
 * hist->moments, out->len equal to hist->len (neighbours of the history are read: not in
 * place; out->moments may be cur->moments). */
int rt_temporal(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                const rt_temporal_frame *out, double *ms);
/* The same with device pointers in the frames, enqueued on `stream`.  No workspace: calls may
 * overlap.  Two history sets ping-pong: this call's `out` (with cur's guides) is the next
 * call's `hist`, and the set before it the next `out`. */
int rt_temporal_dev(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                    const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                    const rt_temporal_frame *out, void *stream);

/* ------------------------------- the same with the history clipped to the frame's colour box */
typedef struct rt_temporal_clamp_params {   /* 32 bytes */
    int32_t radius;    /* 0..3: half-width of the window of the current frame; 0 = no clamp */
    float   gamma;     /* >= 0, finite: half-width of the box in standard deviations */
    int32_t pad[6];    /* zero */
} rt_temporal_clamp_params;
/* rt_temporal with variance clipping (Salvi 2016; Karis 2014): between the history fetch and the
 * blend, a reprojected pixel's history colour c_h is clipped, per channel, to the colour box of
 * the current frame around the pixel, so that a history that has drifted — resampled at every
 * reprojection, shaded for an older eye — cannot stray further than the frame allows.  Every
 * argument of rt_temporal means what it means there; with cp->radius = r >= 1 and unequal
 * cameras, for a pixel (x, y) that found a history (`use` of the rule above):
 *   the window is the current frame's colour v at (x + dx, y + dy), dy = -r..r (outer), dx = -r..r
 *   (inner), every cell inside the image, the centre included; cnt their number, S1 and S2 the
 *   running sums of v and v * v per channel in that order;
 *   m = S1 / cnt, var = max(S2 / cnt - m * m, 0), sd = sqrt(var), lo = m - gamma * sd,
 *   hi = m + gamma * sd, c_h' = c_h < lo ? lo : (c_h > hi ? hi : c_h);
 *   bit c of the pixel's `clipped` value is set when channel c moved (c_h' != c_h);
 *   with moments and a nonzero mask the history's per-sample mean moves along and its variance
 *   stays: y = (c_h0 + c_h1) + c_h2, y' likewise of c_h', mu_1' = max(mu_1 + (y' - y), 0),
 *   v = max(mu_2 - mu_1 * mu_1, 0), mu_2' = v + mu_1' * mu_1'; with a zero mask they are untouched;
 *   n_h is unchanged, and the blend runs on c_h', mu_1', mu_2'.
 * A first frame, bytewise equal cameras (nothing drifts there, and a clamp would bias an exact
 * running mean) and radius 0 are rt_temporal bit for bit, whatever else cp says, with clipped = 0;
 * so is a pixel without history.  `clipped` (nx*ny, or NULL) receives the masks.  The exact float32
 * statement is tests/test_temporal_clamp_spec.py (temporal_clamped_ref).  gamma 0 replaces a
 * history colour outside the window's mean by that mean; a large gamma never binds.
 * No setting is suggested for every scene (DESIGN.md §7j records the sweep): at 4 spp a frame
 * radius 1, gamma 0.5 lowers random_scene's error by 8 % and raises final()'s by 14 %, wider
 * windows hardly bind; radius 0 is the default of the Python layer.
 * Host form: as rt_temporal's; `clipped` is a host pointer; *ms is the kernel's time (where nothing
 * is clamped the mask is zeroed ahead of the timed interval).  Synchronous.
 * RT_ERR_INVALID: every case of rt_temporal, with its message; then, checked before the device
 * is touched and named in rt_last_error(), a null cp, radius outside 0..3, gamma negative, NaN
 * or infinite, a nonzero pad; `clipped` equal to one of the arrays of cur, hist or out (the mask is
 * a buffer of its own). */
int rt_temporal_clamped(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                        const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                        const rt_temporal_clamp_params *cp, const rt_temporal_frame *out, int32_t *clipped, double *ms);
/* The same with device pointers in the frames and for clipped_dev (or NULL), enqueued on
 * `stream`; where nothing is clamped, clipped_dev is zeroed on `stream` ahead of the kernel.  No
 * workspace: calls may overlap; the history sets ping-pong as rt_temporal_dev's. */
int rt_temporal_clamped_dev(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                            const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                            const rt_temporal_clamp_params *cp, const rt_temporal_frame *out, int32_t *clipped_dev,
                            void *stream);

/* ------------------------------- the same with a history for background and edge pixels */
enum { RT_TEMPORAL_SRC_NONE = 0, RT_TEMPORAL_SRC_SURFACE = 1, RT_TEMPORAL_SRC_BACKGROUND = 2,
       RT_TEMPORAL_SRC_EDGE = 4 /* or'ed in: 0 < coverage < 1 */, RT_TEMPORAL_SRC_SAME = 8 /* equal cameras */ };
typedef struct rt_temporal_cover_params {   /* 32 bytes */
    int32_t background;      /* 0 / 1: pixels that miss take history by direction */
    int32_t edges;           /* 0 / 1: partly covered pixels take the class of their dominant part */
    float   sigma_coverage;  /* >= 0, finite: a tap counts only when |c - c_q| <= sigma_coverage */
    int32_t pad[5];          /* zero */
} rt_temporal_cover_params;
/* rt_temporal_clamped with a history for the pixels rt_temporal gives none under unequal cameras:
 * those that look past the geometry and those on a silhouette.  Every argument of
 * rt_temporal_clamped means what it means there (cp is required; radius 0 means no clamp).  With
 * c the pixel's coverage, a pixel belongs to one of two classes or to none:
 *   surf = c == 1 || (edges && c >= 0.5);
 *   back = !surf && background && (c == 0 || (edges && c < 0.5));
 *   neither: no history, the output is the frame bit for bit.
 * A surface pixel's guides are means over samples in which a miss contributes 0, so the hit
 * samples' means are n = normal / c and z = depth / c (IEEE divides; the same bits for c == 1); it
 * is reprojected as rt_temporal does with z as its depth.  A background pixel is a point at
 * infinity: d = dir, the direction through the pixel centre, with no expected depth.  From
 * d . w' < 0 to the four taps and their weights both classes follow rt_temporal's rule.  A tap q
 * with coverage c_q counts when its weight is positive, it is inside the image, hist len[q] > 0,
 * |c - c_q| <= sigma_coverage and
 *   for a surface pixel: c_q == 1 || (edges && c_q >= 0.5), n . (n_q / c_q) >= cos_normal, and
 *     rt_temporal's depth test on z' = |d| and z_q = depth_q / c_q;
 *   for a background pixel: c_q == 0 || (edges && c_q < 0.5), and nothing else.
 * W, the history colour, the per-sample moments and n_h are formed as in rt_temporal; with
 * cp->radius >= 1 rt_temporal_clamped's clamp runs on every pixel that found a history, whatever
 * its class; the blend is rt_temporal's.  `source` (nx*ny, or NULL) receives per pixel where its
 * history came from: RT_TEMPORAL_SRC_NONE without one, else RT_TEMPORAL_SRC_SURFACE or
 * RT_TEMPORAL_SRC_BACKGROUND, with RT_TEMPORAL_SRC_EDGE or'ed in when c is neither 0 nor 1.
 * With vp zeroed (background 0, edges 0, any valid sigma_coverage) this is rt_temporal_clamped bit
 * for bit and source is 1 exactly where a history was used: coverage 1 against coverage 1 passes
 * every new test, so the settings only add pixels and taps.  A first frame is rt_temporal bit for
 * bit with clipped 0 and source 0; so are bytewise equal cameras, with clipped 0 and source
 * RT_TEMPORAL_SRC_SAME where a history was used.  The exact float32 statement is
 * tests/test_temporal_cover_spec.py (temporal_cover_ref).
 * Suggested: background 1, edges 1, sigma_coverage 0.5, no clamp (DESIGN.md §7k records the sweep:
 * over a camera move at 4 spp a frame that lowers final()'s error by 28 %, 98 % of its pixels
 * taking a history instead of 41 %, and random_scene's by 1.4 %; 3 us on rt_temporal's 25 us).
 * Host form: as rt_temporal_clamped's; `source` is a host pointer; *ms is the kernel's time (a
 * first frame's and equal cameras' mask and source are written ahead of the timed interval).
 * RT_ERR_INVALID: every case of rt_temporal_clamped, with its message; then, checked before the
 * device is touched and named in rt_last_error(), a null vp, background or edges other than 0 or
 * 1, sigma_coverage negative, NaN or infinite, a nonzero pad; `source` equal to `clipped` or to one
 * of the arrays of cur, hist or out. */
int rt_temporal_cover(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                      const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                      const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp, const rt_temporal_frame *out,
                      int32_t *clipped, int32_t *source, double *ms);
/* The same with device pointers in the frames and for clipped_dev and source_dev (each may be
 * NULL), enqueued on `stream`; a first frame's and equal cameras' mask and source are written on
 * `stream` ahead of the kernel.  No workspace: calls may overlap; the history sets ping-pong as
 * rt_temporal_dev's. */
int rt_temporal_cover_dev(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                          const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                          const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp,
                          const rt_temporal_frame *out, int32_t *clipped_dev, int32_t *source_dev, void *stream);

/* ------------------------------- ray queries on the caller's own rays */
#define RT_HIT_MISS (-1)
#define RT_HIT_INVALID (-2)
typedef struct rt_ray {      /* 48 bytes */
    float origin[3], t_min;
    float dir[3],    t_max;  /* dir need not be unit length; t is in units of dir */
    float time;              /* moving spheres (sphere.h:81-83); ignored without them */
    float pad[3];            /* ignored */
} rt_ray;
typedef struct rt_hit {      /* 48 bytes */
    int32_t prim;            /* index into rt_scene_desc.prims; RT_HIT_MISS -1; RT_HIT_INVALID -2 */
    int32_t material;        /* that primitive's material index; -1 without a hit */
    float t, depth;          /* hit parameter; t * |dir| (0, 0 without a hit) */
    float normal[3];         /* the hit record's normal, as rt_render_features defines it; 0 without a hit */
    float albedo[3];         /* the hit material's colour, as rt_render_features defines it; (1,1,1) without a hit */
    int32_t pad[2];          /* written as 0 */
} rt_hit;
/* Closest hit.  hits[k] is what hitable_list::hit(r, t_min, t_max, rec) returns for rays[k]
 * over the scene's surfaces, constant media skipped as rt_render_features skips them: the
 * closest hit under each primitive's own acceptance rule — a sphere needs t_min < t < t_max
 * (sphere.h:33), a rect accepts t_min <= t <= t_max (aarect.h:52) — with ties by the list's
 * rule: a later rect wins a tie, a sphere never displaces an earlier hit at equal t.  A t_max
 * of +inf, or at or above FLT_MAX, means the reference's MAXFLOAT.  prim is the index into
 * rt_scene_desc.prims (the descriptor's list index, not a place in the device's arrays),
 * material that primitive's material; normal and albedo are exactly rt_render_features'
 * per-sample values, and depth is t * len(dir) as that pass computes it (the float32 product,
 * len = sqrtf((x*x + y*y) + z*z)).
 * Occlusion.  rt_occluded writes 1 exactly where rt_trace_rays reports prim >= 0, 0 where it
 * reports a miss; its search may stop at the first accepted hit.
 * Invalid rays.  A ray is invalid when origin, dir, time or t_min has a non-finite component,
 * t_max is NaN, dir is (0, 0, 0), or the scene has moving spheres and time lies outside the
 * scene's [time0, time1] (the moving spheres' boxes do not cover it).  It reports
 * RT_HIT_INVALID (255 from rt_occluded) with the other fields as for a miss; the device tests
 * every ray itself, the other rays of the call are not affected.
 * Axis-parallel rays.  A ray with a direction component of exactly 0 is traced like any other.
 * Where a rect is tested its result is outside the parity contract, as in the renders
 * (DESIGN.md §2); on scenes of spheres only it is exact.
 * Arguments, all checked before any HIP call, the scene last: RT_ERR_INVALID for n < 0 or
 * n > 2^31 - 1; n == 0 is RT_OK and touches nothing, whatever the other arguments;
 * RT_ERR_INVALID for null rays or a null output, then for a null scene; RT_ERR_UNSUPPORTED on
 * a scene with a wide BVH (RTNW_BVH_WIDTH 4, 8, 8q) or when the library was linked without
 * the trace unit.
 * The host forms are synchronous and stage rays and results through device buffers kept with
 * the scene, in batches of RTNW_TRACE_BATCH rays (env; default 2^20, at most 2^24); the result
 * does not depend on the batch size.  *ms, when non-NULL, receives the kernels' HIP-event time.
 * The _dev forms take device pointers (16-B aligned rays and hits), need no workspace and
 * only enqueue on `stream` (hipStream_t, NULL = default). */
int rt_trace_rays    (rt_scene *s, const rt_ray *rays, int64_t n, rt_hit *hits, double *ms);   /* host buffers, synchronous */
int rt_trace_rays_dev(rt_scene *s, const rt_ray *rays_dev, int64_t n, rt_hit *hits_dev, void *stream);
int rt_occluded      (rt_scene *s, const rt_ray *rays, int64_t n, uint8_t *out, double *ms);   /* 0 clear, 1 occluded, 255 invalid ray */
int rt_occluded_dev  (rt_scene *s, const rt_ray *rays_dev, int64_t n, uint8_t *out_dev, void *stream);

/* ------------------- radiance queries: the path-traced colour of the caller's own rays */
#define RT_RADIANCE_MAX_SKIP 192   /* the reach of the kernel's drand48 jump table (RT_LCG_JUMPS - 1) */
typedef struct rt_path_ray {      /* 48 bytes, 16-B aligned in the _dev forms */
    float origin[3], time;        /* time: moving spheres (sphere.h:81-83) */
    float dir[3];                 /* need not be unit length */
    uint32_t skip;                /* draws of the sample's stream already spent by the caller, 0..RT_RADIANCE_MAX_SKIP */
    uint32_t pixel, sample;       /* the stream: sample_key(p->seed, pixel, sample), DESIGN.md §3 */
    uint32_t pad[2];              /* ignored */
} rt_path_ray;
typedef struct rt_radiance {      /* 16 bytes */
    float rgb[3];                 /* de_nan(color(ray, world, 0)), main.cpp:25-46, 232-242 */
    int32_t status;               /* 0, or RT_HIT_INVALID */
} rt_radiance;
/* Result.  out[k].rgb is what the megakernel's default (forward-throughput) path computes for
 * one sample whose first segment is rays[k]: the same stages, t_min, max_depth, background and
 * de_nan as a render's sample.  It is the value a work item adds to its partial sum, before
 * any sum over samples or mean: the one-sample work item's own sum 0 + de_nan(color(...)), so
 * a component that is -0 comes back +0, as it does from every render.
 * Main stream.  The sample's drand48 stream is restarted at the key of
 * (p->seed, pixel, sample) and advanced by `skip` draws before the first scatter draws from it.
 * Medium stream.  The sample's medium stream starts at its usual key, derived from the same
 * (p->seed, pixel, sample), with segment 0.  `skip` does not affect it.
 * Key fields are data.  pixel and sample are any uint32_t; nothing relates them to a frame.
 * Parameters used from p: max_depth, t_min, background, seed.  nx, ny, spp, chunk and
 * sample_offset are ignored.  Any flag is RT_ERR_INVALID (there are no right-fold, counting or
 * profiling forms of the query).
 * The ray-tracing identity (the contract).  If rays[k] is the ray camera::get_ray returns for
 * sample `sample` of pixel key `pixel` (the uint32_t j * nx + x of rt_render_params' limits),
 * and skip is the number of draws that sample spent before color(), then out[k].rgb is bitwise
 * that pixel of rt_render_tile with spp = 1, sample_offset = sample and the same seed,
 * max_depth, t_min and background.  The draws spent are 2 jitter draws (main.cpp:305-306), 2
 * per lens-disk candidate including the accepted one (camera.h:49-56, drawn even when the lens
 * radius is 0) and 1 time draw: 5 + 2 * (rejected candidates).
 * skip range.  0..RT_RADIANCE_MAX_SKIP; a larger skip makes that ray invalid.
 * Invalid rays.  A ray is invalid when origin, dir or time has a non-finite component, dir is
 * (0, 0, 0), the scene has moving spheres and time lies outside the scene's [time0, time1], or
 * skip > RT_RADIANCE_MAX_SKIP.  Its record comes back (0, 0, 0, RT_HIT_INVALID); it is never
 * traced; the device tests every ray itself, and the other rays of the call are not affected.
 * Axis-parallel rays are traced like any other, with rt_trace_rays' caveat on rects.
 * Result independence.  A ray's record depends only on its rt_path_ray, the scene and p: not on
 * its position in the call, on n, or on the host form's batches.
 * Arguments, all checked before any HIP call, the scene last, in this order: RT_ERR_INVALID
 * for n < 0 or n > 2^31 - 1; n == 0 is RT_OK and touches nothing, whatever the other
 * arguments; RT_ERR_INVALID for a null p, rays or out, max_depth < 0, a non-finite t_min, a
 * background outside RT_BG_* or any flag; RT_ERR_INVALID for a null scene; RT_ERR_UNSUPPORTED
 * on a scene with a wide BVH (RTNW_BVH_WIDTH 4, 8, 8q) or when the library was linked without
 * the rays unit.
 * The host form is synchronous and stages rays and records through device buffers kept with
 * the scene, in batches of RTNW_RADIANCE_BATCH rays (env; default 2^20, at most 2^24); *ms,
 * when non-NULL, receives the kernels' HIP-event time.  The _dev form takes device pointers
 * (16-B aligned) and only enqueues on `stream` (hipStream_t, NULL = default); like the renders
 * it uses the scene's work counter, so calls on one scene must not overlap each other or a
 * render of that scene. */
int rt_radiance_rays    (rt_scene *s, const rt_render_params *p, const rt_path_ray *rays, int64_t n, rt_radiance *out, double *ms);
int rt_radiance_rays_dev(rt_scene *s, const rt_render_params *p, const rt_path_ray *rays_dev, int64_t n, rt_radiance *out_dev, void *stream);

/* ------------------- lens renders: panorama, fisheye and orthographic cameras */
enum { RT_LENS_PERSPECTIVE = 0, RT_LENS_ORTHOGRAPHIC = 1, RT_LENS_FISHEYE = 2, RT_LENS_EQUIRECT = 3 };
typedef struct rt_lens_params {   /* 32 bytes */
    int32_t model;                /* RT_LENS_* */
    float   fov_deg;              /* FISHEYE: full angle across the image circle, 0 < fov <= 360; else ignored */
    int32_t pad[6];               /* zero */
} rt_lens_params;
/* A camera model on top of rt_camera_desc: the rays of every (pixel, sample) made on the device
 * (rt_lens_rays), and the render that feeds them through the radiance query and reduces the
 * result by the renders' own summation rule (rt_render_lens).  rt_camera_desc (rt_camera_init)
 * supplies the pose origin, u, v, w and the shutter time0, time1; for PERSPECTIVE also
 * lower_left_corner, horizontal, vertical and lens_radius, for ORTHOGRAPHIC horizontal and
 * vertical (the extent of the view).
 * Records.  rt_lens_rays writes the w x h rectangle's records sample-major: record
 * k = (sample - sample_offset) * (w * h) + row * w + col, row 0 the top row, for samples
 * [sample_offset, sample_offset + spp).  Its pixel key is the renders' own, pixel =
 * (ny - 1 - (y0 + row)) * nx + (x0 + col), its stream sample_key(seed, pixel, sample), and with
 * x = x0 + col, j = ny - 1 - (y0 + row) the image coordinates are s = (x + draw0) / nx and
 * t = (j + draw1) / ny, computed as the renders compute them.  The exact float32 statement of
 * every model, operation order included, is tests/test_lens_spec.py:
 *   PERSPECTIVE    camera::get_ray exactly (camera.h:41-56): the lens-disk candidates, then the
 *                  time draw; skip = 5 + 2 * (rejected candidates).
 *   ORTHOGRAPHIC   origin = (origin + (s - 0.5) horizontal) + (t - 0.5) vertical, dir = -w; no
 *                  lens draws; skip = 3.
 *   FISHEYE        equidistant: x = 2s - 1, y = 2t - 1, r = sqrtf(x x + y y), theta = r *
 *                  (fov_deg * float(pi / 360)), dir = (sin theta x / r) u + (sin theta y / r) v -
 *                  cos theta w, and -w at r == 0; skip = 3.  A sample with r > 1 lies outside the
 *                  image circle and has NO RAY: its record carries the direction (0, 0, 0), which
 *                  the queries report as RT_HIT_INVALID with radiance (0, 0, 0).  By design it
 *                  counts in the pixel's mean as black and in the guides as a miss (coverage 0),
 *                  so the corners of a fisheye image are black and the circle's rim is blended.
 *   EQUIRECT       phi = 2 pi (s - 0.5), el = pi (t - 0.5), dir = (cos el sin phi) u + (sin el) v
 *                  - (cos el cos phi) w: the image centre looks along -w, the top row up; skip = 3.
 * Every sine is glibc's sinf, bit for bit (the device's restatement of it); every cosine is that
 * sine of the complementary angle formed from the pixel coordinate: cos el = sin(pi (1 - t)),
 * cos phi = sin(2 pi (0.75 - s)), cos theta = sin(float(pi / 2) - theta).  The time of every
 * model is float(double(time0) + draw * double(time1 - time0)) (camera.h:54); a closed shutter
 * consumes the draw unused.  trace_rays, when non-NULL, receives the same rays as rt_ray:
 * t_min = p->t_min, t_max = +inf, the same time; a no-ray sample keeps its zero direction.
 * Parameters read from p: nx, ny, spp, sample_offset, seed, max_depth, t_min, background; chunk
 * is ignored (there is one add per sample); any flag is RT_ERR_INVALID.
 * Render outputs, row-major h x w.  Every sum runs in float32, in sample order, one add per
 * sample, from 0; the means are the sums times float(1.0 / spp), as rt_render_tile's:
 *   out_rgb      3 floats per pixel: the mean of the samples' rt_radiance rgb;
 *   out_moments  2 floats per pixel (NULL: not wanted): sum y and sum y * y, y = (r + g) + b per
 *                sample, sums as rt_render_tiles_moments writes them at chunk 1;
 *   out_guides   8 floats per pixel (NULL: not wanted), packed as rt_render_features_dev packs
 *                them: the mean of the samples' rt_hit albedo, coverage (1 where prim >= 0),
 *                normal and depth, from rt_trace_rays' search run on trace_rays: asking for the
 *                guides costs one more lane-per-ray pass.
 * Contracts.
 *   Perspective identity: with RT_LENS_PERSPECTIVE the image is rt_render_tile(chunk = 1) bit for
 *     bit, the moments rt_render_tiles_moments(chunk = 1)'s, the guides rt_render_features_dev's.
 *   Composition: for every model rt_render_lens is rt_lens_rays' records fed through
 *     rt_radiance_rays (and its trace_rays through rt_trace_rays) and reduced by the rule above,
 *     bit for bit; invalid rays, axis-parallel rays and rects follow those queries' terms.
 *   Independence: the result depends neither on the batch size nor on the tile split (a tile is
 *     the crop of the frame).
 * Arguments, all checked before any HIP call, in this order, the offending one named in
 * rt_last_error(): RT_ERR_INVALID for a null cam, lens, p or required output (rays; out_rgb); a
 * model outside RT_LENS_*, a nonzero pad, under FISHEYE a fov_deg that is NaN or outside
 * (0, 360]; nx or ny outside 1..65535, spp < 1, sample_offset + spp above 0xFFFFFFFF; a rectangle
 * empty or outside the frame; any flag; max_depth < 0, a non-finite t_min, a background outside
 * RT_BG_*.  The renders then check the scene: RT_ERR_INVALID when it is NULL, RT_ERR_UNSUPPORTED
 * on a wide BVH (RTNW_BVH_WIDTH 4, 8, 8q) or when the library was linked without the lens, rays
 * or (for guides) trace unit, and RT_ERR_INVALID when the scene has moving spheres and the
 * camera's [time0, time1] leaves the scene's span (every sample would come back invalid).
 * The render works in batches of whole sample planes of a pixel block, at most RTNW_LENS_BATCH
 * rays each (env; default 2^21, at most 2^24; any value >= 1 works), in a workspace kept with
 * the scene.  The host forms are synchronous; *ms, when non-NULL, receives the batches' summed
 * HIP-event time.  The _dev forms take device pointers (records and guides 16-B aligned) and only
 * enqueue on `stream` (hipStream_t, NULL = default).  Like the radiance queries a lens render
 * uses the scene's work counter and workspace: calls on one scene must not overlap each other,
 * a render or a query of that scene. */
int rt_lens_rays    (int device, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p,
                     int x0, int y0, int w, int h, rt_path_ray *rays, rt_ray *trace_rays);
int rt_lens_rays_dev(int device, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p,
                     int x0, int y0, int w, int h, rt_path_ray *rays_dev, rt_ray *trace_rays_dev, void *stream);
int rt_render_lens    (rt_scene *s, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p,
                       int x0, int y0, int w, int h, float *out_rgb, float *out_moments, float *out_guides, double *ms);
int rt_render_lens_dev(rt_scene *s, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p,
                       int x0, int y0, int w, int h, float *out_rgb_dev, float *out_moments_dev, float *out_guides_dev,
                       void *stream);

/* Diagnostic: the device's float transcendentals of the path on n host inputs (out: n
 * floats) — fn 0 the megakernel's sinf (texture.h:36, 55), 2 its asinf and 4 its
 * atan2f(a, b) (hitable.h:15-16), all restated from glibc (rt_libm.h); 1, 3, 5 ocml's
 * sinf / asinf / atan2f for comparison.  For the parity tests; not on the render path. */
int rt_math_probe(int fn, const float *a, const float *b, float *out, int64_t n);

/* ------------------------------------------------ multi-GPU
 * One process per GPU.  The root calls rt_dist_unique_id and hands the 128 bytes to
 * every rank (any side channel); each rank calls rt_dist_init (ncclCommInitRank),
 * renders its share of the pixels — by default 8 x 8 pixel blocks dealt along a
 * Hilbert curve (rt_rank_tiles, RT_LAYOUT_BLOCKS), or the interleave of rt_rank_pixels:
 * with world = a x b, rank (ry, rx) renders x = rx (mod a), y = ry (mod b), a
 * sub-sampled copy of the whole view — and ONE ncclGather (rccl.h:745) brings the packed shares
 * to the root, which unpacks them.  The RNG is keyed by (pixel, sample), so the
 * image is bitwise the 1-GPU image for any rank count.                           */
#define RT_DIST_ID_BYTES 128
typedef struct rt_dist rt_dist;   /* one rank's RCCL communicator */
int rt_dist_unique_id(uint8_t id[RT_DIST_ID_BYTES]);             /* ncclGetUniqueId (root only) */
int rt_dist_init(const uint8_t id[RT_DIST_ID_BYTES], int rank, int world, int device, rt_dist **out);
void rt_dist_destroy(rt_dist *d);
/* ncclGather of `count` floats from every rank's send_dev into recv_dev on `root`
 * (world x count floats, rank-major); enqueued on `stream` (hipStream_t, NULL = default). */
int rt_dist_gather(rt_dist *d, const float *send_dev, uint64_t count, float *recv_dev, int root, void *stream);
/* world = a x b, a >= b, as square as possible (8 -> 4 x 2). */
void rt_interleave_factors(int world, int *a, int *b);
/* The pixels of `rank` as 1x1 tiles (4 int32 each) in claim order: bands of 8 rows of
 * the rank's lattice, column by column.  Returns the count (tiles == NULL: count only). */
int64_t rt_rank_pixels(int nx, int ny, int rank, int world, int32_t *tiles, int64_t cap);
/* How a job's pixels are split over the ranks (rt_rank_tiles, rt_dist_set_layout):
 *   RT_LAYOUT_BLOCKS       the image's block x block pixel blocks in Hilbert-curve order,
 *                          block k of the curve to rank k mod world (the default of
 *                          rt_dist_render and bench.py: every rank's blocks spread over
 *                          the view, and a wave's 64 work items stay one 8 x 8 block);
 *   RT_LAYOUT_INTERLEAVED  rt_rank_pixels' pixel interleave;
 *   RT_LAYOUT_LATTICE      the blocks on the interleave's a x b lattice, row-major.
 * The pixels come as 1x1 tiles in claim order (each block column by column).  Returns the
 * count (tiles == NULL: count only), RT_ERR_INVALID for a bad argument or a short buffer;
 * block <= 0 means RT_LAYOUT_BLOCK, a block above 65535 (no frame is larger) is
 * RT_ERR_INVALID.  Replaces main.cpp:299-300's one pixel loop per job. */
#define RT_LAYOUT_BLOCKS 0
#define RT_LAYOUT_INTERLEAVED 1
#define RT_LAYOUT_LATTICE 2
#define RT_LAYOUT_BLOCK 8
int64_t rt_rank_tiles(int nx, int ny, int rank, int world, int layout, int block, int32_t *tiles, int64_t cap);
/* Scatters packed tiles (rt_render_tiles' output layout) into an nx x ny x 3 image. */
int rt_unpack_tiles(const float *packed, const int32_t *tiles, int64_t ntiles, int nx, int ny, float *image);
/* The whole rank job: this rank's pixels -> rt_render_tiles -> rt_dist_gather -> on the
 * root, the full nx x ny x 3 mean image in host memory (`image`; NULL on other ranks).
 * Mean images only: RT_FLAG_SUM_IN / RT_FLAG_SUM_OUT return RT_ERR_INVALID (on every
 * rank alike).  The other flags pass through to rt_render_tiles unchanged, so
 * RT_FLAG_RIGHT_FOLD renders the right-fold image on every rank's share.
 * A rank whose render fails still joins the gather; one that cannot
 * allocate its buffers aborts the communicator (ncclCommAbort, later calls on it fail)
 * and its launcher must stop the peers waiting in the gather. */
int rt_dist_render(rt_dist *d, rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, float *image,
                   rt_stats *stats);
/* The split rt_dist_render uses (RT_LAYOUT_*; RT_LAYOUT_BLOCKS unless set).  Every rank of
 * a job must set the same layout.  The gathered image is the same for every layout. */
int rt_dist_set_layout(rt_dist *d, int layout);

/* ----------------------------------------------------- resolve (main.cpp:314-330) */
/* sqrt gamma + int(255.99*c) + clamp to 255, per channel (main.cpp:316-325). */
void rt_quantize(const float *mean_rgb, int64_t n_pixels, uint8_t *rgb);
/* P3 text of main.cpp:297,327-330; returns the byte count (writes when buf != NULL and cap suffices). */
int64_t rt_ppm_text(const uint8_t *rgb, int nx, int ny, char *buf, int64_t cap);

/* ------------------------------------------- checkpoint / resume
 * A progressive render keeps per-pixel SUMS (RT_FLAG_SUM_OUT) and resumes from them
 * (RT_FLAG_SUM_IN with sample_offset = samples_done): bitwise the same image as an
 * uninterrupted render.  The file holds this header, `count` floats in the packed
 * tile layout of rt_render_tiles, and a checksum; it is replaced atomically.       */
#define RT_CHECKPOINT_MAGIC 0x4B435452u   /* "RTCK" */
#define RT_CHECKPOINT_VERSION 1u
typedef struct rt_checkpoint {
    uint32_t magic, version;      /* set by rt_checkpoint_write */
    int32_t nx, ny;               /* full image */
    uint32_t samples_done;        /* the sums hold samples [0, samples_done) of every pixel */
    int32_t max_depth, background;
    float t_min;
    uint64_t seed;                /* counter-RNG key of the render */
    uint64_t job_hash;            /* caller's identification of the scene / tiles */
    uint64_t count;               /* floats that follow (3 per pixel) */
} rt_checkpoint;
int rt_checkpoint_write(const char *path, const rt_checkpoint *hdr, const float *sums);
/* sums == NULL reads the header only; otherwise cap = capacity of sums in floats. */
int rt_checkpoint_read(const char *path, rt_checkpoint *hdr, float *sums, uint64_t cap);

/* ------------------------------------------------ host scene construction */
/* Builds one of the reference's scenes with the host API (random_scene, random_motion,
 * cornell_box, cornell_smoke, final, simple_light, two_spheres, test) exactly as a
 * fresh reference process would (drand48 state 0, Perlin static init first) and
 * returns its flattened descriptor (free with rt_scene_desc_free). */
int rt_builtin_scene_desc(const char *name, rt_scene_desc **out);
void rt_scene_desc_free(rt_scene_desc *d);
/* Leaf dump in the text format of oracle/ref_harness.cpp --dump (for parity tests). */
int64_t rt_scene_desc_dump(const rt_scene_desc *d, char *buf, int64_t cap);

const char *rt_last_error(void);
const char *rt_version(void);

#ifdef __cplusplus
}
#endif
#endif
