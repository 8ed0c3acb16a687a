/* oracle/rt_oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C99) of the reference path tracer's hot path:
 * main.cpp:299-332 sample loop → camera::get_ray (camera.h:41-56) → color()
 * recursion (main.cpp:25-46) → hitable_list / sphere / moving_sphere / aarect /
 * box / flip_normals / translate / rotate_y / constant_medium hit → material
 * scatter (material.h) → texture value (texture.h, perlin.h).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library, and only as the checker.  The product (librt_hip.so) never links
 * or calls it.
 *
 * Parity pin: in canonical-RNG / media-inline / right-fold mode the restatement
 * reproduces the reference's own PPM bit-for-bit (MD5 of oracle/_ref/ref_render,
 * the reference compiled from /root/reference; fixtures in tests/golden/).
 */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H
#include <stdint.h>

#include "../include/rt_hip.h"   /* layouts only (rt_scene_desc, rt_camera_desc): nothing of librt_hip is linked */

#ifdef __cplusplus
extern "C" {
#endif

enum oracle_scene {
    ORACLE_SCENE_RANDOM = 0,        /* main.cpp:49-85 */
    ORACLE_SCENE_RANDOM_MOTION = 1, /* TNW/Chapter01:36-67 with main.cpp texture API */
    ORACLE_SCENE_CORNELL = 2,       /* main.cpp:148-166 */
    ORACLE_SCENE_CORNELL_SMOKE = 3, /* main.cpp:169-188 */
    ORACLE_SCENE_FINAL = 4,         /* main.cpp:190-230 */
    ORACLE_SCENE_SIMPLE_LIGHT = 5,  /* main.cpp:122-133 */
    ORACLE_SCENE_TWO_SPHERES = 6,   /* main.cpp:99-110 */
    ORACLE_SCENE_TEST = 7,          /* main.cpp:135-145 */
    ORACLE_SCENE_EARTH = 8,         /* main.cpp:87-97 (image set by oracle_set_image) */
    ORACLE_SCENE_EDGE_EMPTY = 9,    /* edge cases of the tests (ref_harness.cpp edge_*):  no objects */
    ORACLE_SCENE_EDGE_SINGLE = 10,  /*   one sphere (the BVH is a single leaf) */
    ORACLE_SCENE_EDGE_DEGENERATE = 11, /* zero/negative radii, zero-width rect, zero shutter span, density 0 / 1e30 */
    ORACLE_SCENE_EDGE_CHAINS = 12   /*   instance chains (flip between transforms, 6 ops), nested checkers over noise,
                                         metal / dielectric rects, a medium in a translated sphere */
};

enum oracle_camera {
    ORACLE_CAM_CORNELL = 0,   /* main.cpp:254-259 */
    ORACLE_CAM_RANDOM = 1,    /* main.cpp:263-267 */
    ORACLE_CAM_FINAL_ALT = 2  /* main.cpp:271-276 */
};

typedef struct oracle_params {
    int32_t scene;
    int32_t nx, ny, ns;
    int32_t max_depth;      /* scatter while depth < max_depth (main.cpp:34 uses 50) */
    int32_t background;     /* 0 black (main.cpp:44), 1 sky (TNW/Chapter03:29-31) */
    float tmin;             /* main.cpp:27 uses 0.001 */
    int32_t camera;
    int32_t rng;            /* 0 canonical drand48 stream, 1 counter streams */
    int32_t media_after;    /* 0: media tested in list order (reference); 1: after surfaces (kernel) */
    int32_t forward;        /* 0: right-fold recursion (reference); 1: forward throughput (kernel) */
    int32_t chunk;          /* samples per partial sum; 0 = all ns in one sequential sum */
    int32_t x0, y0, w, h;   /* output rectangle in image coords (y down); w == 0: whole image */
    int32_t threads;        /* counter mode only; <=0: 1 */
    uint32_t sample_offset; /* counter mode: first sample index */
    uint32_t pad_;
    uint64_t seed;          /* counter mode key */
} oracle_params;

typedef struct oracle_stats {
    double samples;
    double segments;        /* rays traced (world hit calls) */
    double seconds;         /* wall time of the pixel loop */
} oracle_stats;

/* Renders the rectangle; out_mean = h*w*3 floats of linear mean radiance
 * (after `col /= float(ns)`, before gamma), rows top-down.  Returns 0 on success. */
int oracle_render(const oracle_params *p, float *out_mean, oracle_stats *stats);

/* The same render of any scene descriptor (include/rt_hip.h) seen through the camera as
 * given: the object tree is rebuilt from the descriptor (each primitive under its flip and
 * its instance chain, ops[0] outermost; each medium at its `order` position over the list
 * of its boundary primitives, its draw ordinal its index), with the descriptor's textures,
 * materials, images and Perlin tables (copied per call: no process-wide state).  p->scene
 * and p->camera are ignored; counter RNG only (p->rng == 0 returns -4: the canonical stream
 * is a property of a scene the oracle built itself).  -2: a malformed descriptor — what
 * rt_scene_create's validation refuses (missing Perlin tables included), and media whose
 * `order` decreases along the array: they are "in list order" (rt_hip.h), and a tree built
 * from unsorted ones would not be the list the fields state. */
int oracle_render_desc(const rt_scene_desc *d, const rt_camera_desc *cam, const oracle_params *p, float *out_mean,
                       oracle_stats *stats);

/* First-hit mode: for every camera sample oracle_render_desc traces (same key, jitter, lens
 * and time draws) the closest surface hit under hitable_list's rule, media skipped — what
 * rt_render_features averages (rt_hip.h).  Arrays are [h][w][ns] (x 3 for normal, albedo):
 * prim the index in d->prims (-1 on a miss), depth t * |direction| (0), normal the hit
 * record's (0, 0, 0), albedo the hit material's colour ((1, 1, 1) on a miss). */
int oracle_first_hits_desc(const rt_scene_desc *d, const rt_camera_desc *cam, const oracle_params *p, int32_t *prim,
                           float *depth, float *normal, float *albedo);

/* Caller-supplied rays (what rt_trace_rays and rt_radiance_rays answer, rt_hip.h): no camera.
 *
 * oracle_trace_rays_desc: for each rt_ray, hitable_list::hit(ray(origin, dir, time), t_min,
 * min(t_max, MAXFLOAT), rec) on the tree oracle_render_desc builds, media skipped.  prim, depth,
 * normal and albedo as oracle_first_hits_desc reports them, and t the hit record's (0 on a miss);
 * arrays of n (x 3).  No validity rule is restated: the callers send valid rays only.
 *
 * oracle_radiance_rays_desc: for each rt_path_ray the sample stream is restarted at
 * sample_key(p->seed, pixel, sample) and advanced by `skip` draws, the medium stream starts at
 * its usual key with segment 0, and rgb[3] = 0 + de_nan(color(ray, world, 0)) with p's tmin,
 * max_depth, background, media_after and forward (the one-sample sum of a render: -0 comes back
 * +0).  Of p only those, seed and threads are read.
 *
 * oracle_trace_rays / oracle_radiance_rays: the same over a built-in scene (`scene`, p->scene),
 * which is what pins both to the reference (tests/golden rays_*).  Their prim is the leaf's
 * place in list order, depth first, media left out.
 * All return 0, -1 for a null argument, -2 for a scene that cannot be built. */
int oracle_trace_rays_desc(const rt_scene_desc *d, const rt_ray *rays, int64_t n, int threads, int32_t *prim, float *t,
                           float *depth, float *normal, float *albedo);
int oracle_radiance_rays_desc(const rt_scene_desc *d, const oracle_params *p, const rt_path_ray *rays, int64_t n, float *rgb);
int oracle_trace_rays(int scene, const rt_ray *rays, int64_t n, int threads, int32_t *prim, float *t, float *depth,
                      float *normal, float *albedo);
int oracle_radiance_rays(const oracle_params *p, const rt_path_ray *rays, int64_t n, float *rgb);

/* Quantises a mean-radiance buffer exactly like main.cpp:315-328 into RGB bytes. */
void oracle_quantize(const float *mean, int n_pixels, uint8_t *rgb);

/* Writes the P3 text of main.cpp:297,327-330 into buf (returns bytes needed). */
long oracle_ppm_text(const uint8_t *rgb, int nx, int ny, char *buf, long cap);

/* Perlin tables as generated by perlin.h:82-111 from a fresh drand48 state. */
void oracle_perlin_tables(float *ranvec768, int32_t *perm768);

/* n values of the canonical (glibc-compatible) drand48 stream from state x0. */
void oracle_drand48(uint64_t x0, int n, double *out);

/* n values of the counter sample stream for (seed, pixel, sample). */
void oracle_counter_draws(uint64_t seed, uint32_t pixel, uint32_t sample, int n, double *out);
double oracle_medium_draw(uint64_t seed, uint32_t pixel, uint32_t sample, int bounce, int medium, int nmedia);

/* oracle_render that also marks, in axis[h * w] (may be NULL), the pixels one of whose rays, at
 * any bounce, had a direction component of exactly 0 (an axis-parallel ray: a rect's hit divides
 * by that component).  The parity tests use the mask to leave such pixels out of a comparison. */
int oracle_render_axis(const oracle_params *p, float *out_mean, uint8_t *axis, oracle_stats *stats);

/* Texels for earth()'s image_texture, as stbi_load returned them (main.cpp:93).
 * The oracle keeps a copy; nn is the file's channel count (the texture reads stride 3). */
void oracle_set_image(const uint8_t *data, int nx, int ny, int nn);

/* Text dump of the scene's leaf primitives (format of oracle/ref_harness.cpp --dump). */
long oracle_scene_dump(int scene, char *buf, long cap);

#ifdef __cplusplus
}
#endif
#endif
