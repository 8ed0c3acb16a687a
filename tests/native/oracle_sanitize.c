/* tests/native/oracle_sanitize.c — runs the oracle restatement (oracle/rt_oracle.c,
 * test infrastructure) under AddressSanitizer + UndefinedBehaviorSanitizer
 * (tests/test_sanitizers.py): every scene, both RNG modes and both media orders, a
 * clipped output rectangle, the quantiser, the PPM writer and the RNG helpers; and the
 * descriptor entry points (oracle_render_desc, oracle_first_hits_desc) on a hand-made
 * descriptor with every primitive, texture and material kind, a 6-op chain and 70 media;
 * all three render entry points at the ABI's limits (limits_check); and the entries for
 * caller-supplied rays with their built-in twins (rays_check).
 * Exit 0 = every render returned 0 and no sanitizer fired. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_oracle.h"

/* A descriptor of 5 primitives (one of each kind, two under a 6-op chain), all four texture
 * kinds, all five material kinds and 70 media over two boundary spheres each (past the 64 the
 * oracle's media list once held), rendered in both orders and in first-hit mode. */
static rt_scene_desc g_desc;     /* desc_check's descriptor and camera, kept for limits_check */
static rt_camera_desc g_cam;

static int desc_check(void) {
    enum { NMED = 70 };
    static rt_prim prims[5], bprims[2 * NMED];
    static rt_medium media[NMED];
    static rt_material mats[6];
    static rt_texture texs[4];
    static rt_instance inst[1];
    static rt_image images[1];
    static uint8_t texels[3 * 2 * 3 + 4];
    static float ranvec[768];
    static int32_t perm[768];
    int bad = 0;
    oracle_perlin_tables(ranvec, perm);
    for (int i = 0; i < (int)sizeof texels; i++) texels[i] = (uint8_t)(i * 53);
    images[0].offset = 4; images[0].nx = 2; images[0].ny = 3;
    texs[0].kind = RT_TEX_CONSTANT; texs[0].color[0] = 0.8f; texs[0].color[1] = 0.5f; texs[0].color[2] = 0.2f;
    texs[1].kind = RT_TEX_NOISE; texs[1].scale = 2.0f;
    texs[2].kind = RT_TEX_IMAGE; texs[2].image = 0;
    texs[3].kind = RT_TEX_CHECKER; texs[3].even = 1; texs[3].odd = 2;
    mats[0].kind = RT_MAT_LAMBERTIAN; mats[0].texture = 3;
    mats[1].kind = RT_MAT_METAL; mats[1].texture = -1; mats[1].albedo[0] = mats[1].albedo[1] = mats[1].albedo[2] = 0.9f; mats[1].fuzz = 0.3f;
    mats[2].kind = RT_MAT_DIELECTRIC; mats[2].texture = -1; mats[2].ref_idx = 1.5f;
    mats[3].kind = RT_MAT_DIFFUSE_LIGHT; mats[3].texture = 0;
    mats[4].kind = RT_MAT_ISOTROPIC; mats[4].texture = 0;
    mats[5].kind = RT_MAT_LAMBERTIAN; mats[5].texture = 2;
    inst[0].nops = 6;
    const float ops[6][4] = {{RT_OP_TRANSLATE, 0.5f, 0.2f, 0}, {RT_OP_ROTATE_Y, 0.5f, 0.8660254f, 0}, {RT_OP_FLIP, 0, 0, 0},
                             {RT_OP_TRANSLATE, 0, 0.1f, 0.2f}, {RT_OP_ROTATE_Y, -0.2588190f, 0.9659258f, 0}, {RT_OP_FLIP, 0, 0, 0}};
    memcpy(inst[0].ops, ops, sizeof ops);
    const float geo[5][9] = {{0, -100, 0, 100}, {1, 0.5f, 0, 1.2f, 0.7f, 0, 0, 1, 0.5f}, {-1, 1, 0, 2, -1.5f},
                             {-2, 2, -2, 2, 3}, {0, 1.5f, -1, 1, -2}};
    for (int i = 0; i < 5; i++) {
        prims[i].kind = i; prims[i].material = i == 3 ? 3 : (i == 4 ? 5 : i); prims[i].instance = (i == 2 || i == 4) ? 0 : -1;
        prims[i].flip = i == 3;
        memcpy(prims[i].p, geo[i], sizeof geo[i]);
    }
    for (int m = 0; m < NMED; m++) {
        for (int k = 0; k < 2; k++) {
            rt_prim *b = &bprims[2 * m + k];
            b->kind = RT_PRIM_SPHERE; b->material = 2; b->instance = k ? 0 : -1;
            b->p[0] = -2.0f + 0.06f * m + 0.3f * k; b->p[1] = 0.6f; b->p[2] = 1.0f; b->p[3] = 0.5f;
        }
        media[m].boundary_first = 2 * m; media[m].boundary_count = 2; media[m].density = 0.2f + 0.05f * m;
        media[m].material = 4; media[m].order = m * 6 / NMED;   /* list order: never decreasing, 0..5 */
    }
    rt_scene_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = RT_ABI_VERSION;
    d.nprims = 5; d.nboundary = 2 * NMED; d.nmedia = NMED; d.nmaterials = 6; d.ntextures = 4; d.ninstances = 1;
    d.prims = prims; d.boundary_prims = bprims; d.media = media; d.materials = mats; d.textures = texs; d.instances = inst;
    d.perlin_ranvec = ranvec; d.perlin_perm = perm; d.time0 = 0; d.time1 = 1;
    d.nimages = 1; d.images = images; d.image_data = texels; d.image_bytes = (int64_t)sizeof texels;
    rt_camera_desc c;
    memset(&c, 0, sizeof c);
    c.origin[0] = 0; c.origin[1] = 1.5f; c.origin[2] = 8;
    c.lower_left_corner[0] = -3; c.lower_left_corner[1] = -0.5f; c.lower_left_corner[2] = 0;
    c.horizontal[0] = 6; c.vertical[1] = 4; c.u[0] = 1; c.v[1] = 1; c.w[2] = 1;
    c.lens_radius = 0.05f; c.time0 = 0; c.time1 = 1;
    static float img[12 * 8 * 3], depth[12 * 8 * 2], nrm[12 * 8 * 2 * 3], alb[12 * 8 * 2 * 3];
    static int32_t prim[12 * 8 * 2];
    for (int mode = 0; mode < 3; mode++) {
        oracle_params p;
        memset(&p, 0, sizeof p);
        p.nx = 12; p.ny = 8; p.ns = 2; p.max_depth = 50; p.background = 1; p.tmin = 0.001f; p.rng = 1;
        p.media_after = mode != 0; p.forward = mode == 2; p.chunk = mode; p.threads = 2; p.seed = 9;
        if (mode == 1) { p.x0 = 2; p.y0 = 1; p.w = 7; p.h = 5; }
        if (oracle_render_desc(&d, &c, &p, img, NULL) != 0) { printf("descriptor mode %d: render failed\n", mode); bad++; }
        if (oracle_first_hits_desc(&d, &c, &p, prim, depth, nrm, alb) != 0) { printf("descriptor mode %d: first hits failed\n", mode); bad++; }
    }
    oracle_params q;
    memset(&q, 0, sizeof q);
    q.nx = 4; q.ny = 4; q.ns = 1; q.rng = 0;
    if (oracle_render_desc(&d, &c, &q, img, NULL) != -4) { printf("descriptor: the canonical stream was not refused\n"); bad++; }
    q.rng = 1;
    prims[1].material = 99;   /* malformed: refused, nothing leaked */
    if (oracle_render_desc(&d, &c, &q, img, NULL) != -2) { printf("descriptor: a bad material index was not refused\n"); bad++; }
    prims[1].material = 1;
    media[3].order = 5;       /* media out of list order: refused */
    if (oracle_render_desc(&d, &c, &q, img, NULL) != -2) { printf("descriptor: unsorted media were not refused\n"); bad++; }
    media[3].order = 3 * 6 / NMED;
    d.perlin_perm = NULL;     /* as rt_scene_create: missing Perlin tables */
    if (oracle_render_desc(&d, &c, &q, img, NULL) != -2) { printf("descriptor: missing Perlin tables were not refused\n"); bad++; }
    d.perlin_perm = perm;
    g_desc = d;
    g_cam = c;
    return bad;
}

/* The ABI's numeric limits (include/rt_hip.h): 8 x 8 tiles in the corners and at the centre of
 * a 65535 x 65535 frame (the centre tile holds row j = 32768 and column 32768, where the pixel
 * key j * nx + x reaches 2^31; from j = 32769 on j * nx passes INT_MAX), the last sample
 * indices (sample_offset = 0xFFFFFFF0) and a seed of all ones, through oracle_render,
 * oracle_render_desc and oracle_first_hits_desc. */
static int limits_check(void) {
    enum { N = 65535, T = 8, NS = 3 };
    static const int at[5][2] = {{0, 0}, {N - T, 0}, {0, N - T}, {N - T, N - T}, {32764, 32763}};
    static float img[T * T * 3], depth[T * T * NS], nrm[T * T * NS * 3], alb[T * T * NS * 3];
    static int32_t prim[T * T * NS];
    static uint8_t axis[T * T];
    int bad = 0;
    for (int t = 0; t < 5; t++)
        for (int fold = 0; fold < 2; fold++) {
            oracle_params p;
            memset(&p, 0, sizeof p);
            p.scene = ORACLE_SCENE_RANDOM; p.camera = ORACLE_CAM_RANDOM; p.background = 1;
            p.nx = N; p.ny = N; p.ns = NS; p.max_depth = 8; p.tmin = 0.001f; p.rng = 1;
            p.media_after = 1; p.forward = !fold; p.chunk = 2; p.threads = 2;
            p.x0 = at[t][0]; p.y0 = at[t][1]; p.w = T; p.h = T;
            p.sample_offset = 0xFFFFFFF0u; p.seed = ~(uint64_t)0;
            oracle_stats st;
            if (oracle_render_axis(&p, img, axis, &st) != 0) { printf("limits: tile %d fold %d: render failed\n", t, fold); bad++; }
            for (int i = 0; i < T * T; i++) if (axis[i] > 1) { printf("limits: tile %d: the axis mask is not 0 or 1\n", t); bad++; break; }
            float sum = 0;
            for (int i = 0; i < T * T * 3; i++) sum += img[i];
            if (!(sum > 0)) { printf("limits: tile %d fold %d: a black tile under the sky\n", t, fold); bad++; }
            p.scene = -1; p.max_depth = 50;
            if (oracle_render_desc(&g_desc, &g_cam, &p, img, NULL) != 0) { printf("limits: tile %d: descriptor render failed\n", t); bad++; }
            if (oracle_first_hits_desc(&g_desc, &g_cam, &p, prim, depth, nrm, alb) != 0) { printf("limits: tile %d: first hits failed\n", t); bad++; }
        }
    return bad;
}

/* The entries for caller-supplied rays on a small batch: rays from inside and outside desc_check's
 * descriptor with both signs of t_min, a finite and an infinite t_max and the ends of the shutter;
 * records with skip 0 and 192 and the ends of the pixel and sample range, in both fold orders
 * and both media orders; the same through the built-in twins; and n = 0 with null arrays. */
static int rays_check(void) {
    enum { N = 24 };
    static rt_ray rays[N];
    static rt_path_ray paths[N];
    static int32_t prim[N];
    static float t[N], depth[N], nrm[N * 3], alb[N * 3], rgb[N * 3];
    int bad = 0, hits = 0;
    for (int i = 0; i < N; i++) {
        const float o[3] = {-2.0f + 0.35f * (float)(i % 12), 0.4f + 0.1f * (float)(i % 5), i < 12 ? 6.0f : 0.9f};
        const float d[3] = {0.11f * (float)(i % 7) - 0.3f, 0.07f - 0.05f * (float)(i % 3), i % 4 == 3 ? 0.8f : -1.0f};
        memset(&rays[i], 0, sizeof rays[i]);
        memset(&paths[i], 0, sizeof paths[i]);
        for (int k = 0; k < 3; k++) { rays[i].origin[k] = paths[i].origin[k] = o[k]; rays[i].dir[k] = paths[i].dir[k] = d[k]; }
        rays[i].t_min = i % 3 == 2 ? -0.5f : (i % 3 ? 0.0f : 0.001f);
        rays[i].t_max = i % 5 == 4 ? 3.0f : 1.0f / 0.0f;
        rays[i].time = paths[i].time = i % 2 ? 1.0f : 0.0f;
        paths[i].skip = i % 3 == 0 ? 0u : (i % 3 == 1 ? 192u : 5u);
        paths[i].pixel = i % 4 == 0 ? 0u : (i % 4 == 1 ? 0xFFFFFFFFu : 77u * (uint32_t)i);
        paths[i].sample = i % 5 == 0 ? 0xFFFFFFFFu : (uint32_t)i;
    }
    if (oracle_trace_rays_desc(&g_desc, rays, N, 2, prim, t, depth, nrm, alb) != 0) { printf("rays: descriptor trace failed\n"); bad++; }
    for (int i = 0; i < N; i++) hits += prim[i] >= 0;
    if (hits == 0 || hits == N) { printf("rays: %d of %d rays hit\n", hits, N); bad++; }
    if (oracle_trace_rays(ORACLE_SCENE_EDGE_CHAINS, rays, N, 1, prim, t, depth, nrm, alb) != 0) { printf("rays: built-in trace failed\n"); bad++; }
    for (int mode = 0; mode < 2; mode++) {
        oracle_params p;
        memset(&p, 0, sizeof p);
        p.scene = ORACLE_SCENE_EDGE_CHAINS; p.max_depth = mode ? 50 : 1; p.background = mode; p.tmin = 0.001f; p.rng = 1;
        p.media_after = mode; p.forward = mode; p.threads = 2; p.seed = mode ? ~(uint64_t)0 : 9;
        if (oracle_radiance_rays_desc(&g_desc, &p, paths, N, rgb) != 0) { printf("rays: descriptor radiance %d failed\n", mode); bad++; }
        if (oracle_radiance_rays(&p, paths, N, rgb) != 0) { printf("rays: built-in radiance %d failed\n", mode); bad++; }
        for (int i = 0; i < 3 * N; i++) if (!(rgb[i] >= 0)) { printf("rays: mode %d: component %d is negative or NaN\n", mode, i); bad++; break; }
        if (oracle_radiance_rays_desc(&g_desc, &p, NULL, 0, NULL) != 0 || oracle_radiance_rays_desc(&g_desc, &p, NULL, 1, rgb) != -1) {
            printf("rays: radiance argument checks\n"); bad++;
        }
    }
    if (oracle_trace_rays_desc(&g_desc, NULL, 0, 1, NULL, NULL, NULL, NULL, NULL) != 0 ||
        oracle_trace_rays_desc(NULL, rays, N, 1, prim, t, depth, nrm, alb) != -1 ||
        oracle_trace_rays(99, rays, N, 1, prim, t, depth, nrm, alb) != -2) { printf("rays: trace argument checks\n"); bad++; }
    return bad;
}

int main(void) {
    int bad = desc_check();
    bad += limits_check();
    bad += rays_check();
    static float img[24 * 16 * 3];
    static uint8_t rgb[24 * 16 * 3];
    static char text[24 * 16 * 16 + 64];
    for (int scene = 0; scene <= ORACLE_SCENE_EDGE_CHAINS; scene++) {
        if (scene == ORACLE_SCENE_EARTH) {   /* a synthetic 5x3 RGBA image for the texture */
            static uint8_t tex[5 * 3 * 4];
            for (int i = 0; i < (int)sizeof tex; i++) tex[i] = (uint8_t)(i * 37);
            oracle_set_image(tex, 5, 3, 4);
        }
        for (int mode = 0; mode < 2; mode++) {
            oracle_params p;
            memset(&p, 0, sizeof p);
            p.scene = scene;
            p.nx = 24; p.ny = 16; p.ns = 2;
            p.max_depth = 50;
            p.background = scene == ORACLE_SCENE_RANDOM || scene == ORACLE_SCENE_RANDOM_MOTION ||
                           scene == ORACLE_SCENE_EARTH || scene == ORACLE_SCENE_TWO_SPHERES;
            p.tmin = 0.001f;
            p.camera = scene == ORACLE_SCENE_CORNELL || scene == ORACLE_SCENE_CORNELL_SMOKE ? ORACLE_CAM_CORNELL
                     : scene == ORACLE_SCENE_FINAL ? ORACLE_CAM_FINAL_ALT : ORACLE_CAM_RANDOM;
            p.rng = mode;
            p.media_after = mode;
            p.forward = mode;
            p.chunk = mode ? 1 : 0;
            if (mode) { p.x0 = 3; p.y0 = 2; p.w = 11; p.h = 9; }
            p.threads = 1;
            p.seed = 5;
            oracle_stats st;
            if (oracle_render(&p, img, &st) != 0) { printf("scene %d mode %d: render failed\n", scene, mode); bad++; }
            const int n = mode ? 11 * 9 : 24 * 16;
            oracle_quantize(img, n, rgb);
            const long need = oracle_ppm_text(rgb, mode ? 11 : 24, mode ? 9 : 16, text, (long)sizeof text);
            if (need <= 0 || need > (long)sizeof text) { printf("scene %d: ppm %ld\n", scene, need); bad++; }
        }
    }
    double d[64];
    oracle_drand48(0, 64, d);
    oracle_counter_draws(1, 2, 3, 64, d);
    (void)oracle_medium_draw(1, 2, 3, 4, 5, 6);
    float ranvec[768];
    int32_t perm[768];
    oracle_perlin_tables(ranvec, perm);
    static char dump[1 << 20];
    for (int scene = 0; scene <= ORACLE_SCENE_EDGE_CHAINS; scene++)
        if (oracle_scene_dump(scene, dump, (long)sizeof dump) <= 0 && scene != ORACLE_SCENE_EDGE_EMPTY) {
            printf("scene %d: dump failed\n", scene);
            bad++;
        }
    printf(bad ? "FAILED %d\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
