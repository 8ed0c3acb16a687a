// rt_megakernel.h — persistent path-tracing megakernel for gfx950 (MI355X): the kernel
// template alone.  The units that instantiate it (rt_kernel.hip, rt_kernel_fold.hip,
// rt_kernel_rays.hip; rt_kernel_knobs.hip for the knob test) include it, and launch it
// through rt_kernel_launch.h.
//
// Device restatement of the reference's hot path:
//   sample loop        main.cpp:299-313   (jitter, get_ray, color, de_nan, col += temp)
//   camera::get_ray    camera.h:41-56
//   color()            main.cpp:25-46     (iterative: throughput * emitted)
//   closest hit        hitable_list.h:20-32 via a BVH2 with exact list-order tie-breaking
//   sphere / moving_sphere / xy|xz|yz_rect / box / flip_normals / translate / rotate_y
//   constant_medium    constant_medium.h:26-50 (evaluated after the surface search)
//   material::scatter  material.h:16-151 ; texture::value texture.h:16-59 ; perlin.h:25-74
//
// Execution model (wave64, CDNA4):
//   * persistent workgroups (16 waves, one per CU, with the BVH2 in LDS; 4 waves with
//     it in HBM; 4 for the flat scan); each LANE owns one camera path at a time and
//     regenerates a new camera sample as soon as its path terminates, so lanes stay
//     busy across bounces (path regeneration) instead of idling until the longest
//     path of the wave finishes;
//   * work = (chunk of `chunk` samples) x (pixel), one sample by default (short items
//     keep a wave's lanes on neighbouring pixels); a wave claims A.claim (<= 512)
//     work items per atomic (one global atomic per claim) and hands them
//     to the lanes that need work with a ballot + mbcnt prefix count;
//   * each item's radiance is summed in registers and stored once into a partial-sum
//     slab [chunk][pixel]; rt_resolve sums the chunks in order (deterministic, no
//     float atomics, independent of the number of GPUs; with one sample per item
//     it is the reference's own `col += temp` order);
//   * the BVH traversal stack lives in LDS, laid out [wave][depth][lane] so every
//     push/pop of a wave is one conflict-free LDS access (16-bit entries with the BVH2
//     in LDS, rt_device.h stk16_*);
//   * ball waves (stage 6, final()'s variant): the workgroup's last A.ball_waves waves
//     gather, through two LDS path pools, the paths whose segments start inside the
//     dense medium's ball, whose closest-hit searches end at the medium cell's few
//     primitives without a BVH descent, so those waves skip the traversal stage;
//   * nodes, primitives and materials are 16-B records read with dwordx4 loads.
//
// Arithmetic follows the reference's float/double promotions; the file is compiled
// with -ffp-contract=off so no FMA is introduced where the reference has none (the
// BVH slab test, which decides nothing about the result, uses explicit fmaf).
#pragma once
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "rt_device.h"

namespace {

// Minimum waves per SIMD the register allocation must allow (launch_bounds second
// argument; 4 -> <= 128 VGPRs -> 16 waves per CU).  5 waves (96 VGPRs) spill 63
// VGPRs and run 24% slower.

// partial sums in the slab: rgb, 12 B per work item (16-B float4 records until round 3)
#define RT_SLAB_FLOATS 3
// Shade once this many lanes of a wave have their closest hit (see stage 3).
#ifndef RT_READY_BATCH
#define RT_READY_BATCH 48
#endif

// Node steps per descent exit check outside the instance variant (rt_device.h descend).
#ifndef RT_DESCEND_STEPS
#define RT_DESCEND_STEPS 2
#endif


// A wave whose claims found the pool dry and that holds at most this many live paths
// runs latency-first (descend's tail cut off)
#ifndef RT_DRY_LANES
#define RT_DRY_LANES 16
#endif


// Pre-made sample starts per wave (refill): one per lane.
#define RT_PRE 64

// Path pools of the ball waves (stage 6): paths whose segment starts inside the medium
// cell's ball, and paths that left it, waiting in LDS for a wave of their kind (80 B each)
#ifndef RT_BALL_POOL
#define RT_BALL_POOL 80
#endif
#ifndef RT_NORM_POOL
#define RT_NORM_POOL 64
#endif
typedef unsigned U4p __attribute__((ext_vector_type(4)));

#ifndef RT_WAVES_PER_SIMD
#define RT_WAVES_PER_SIMD 4
#endif

// kCount: visit counters (RT_FLAG_COUNT).  kProf: wave-level s_memtime stamps per
// stage (RT_FLAG_PROFILE, a diagnostic build whose timing is never quoted).
// Lane phases of the batched state machine below.
// PH_PARK (ball waves): a new segment the medium cell did not decide, waiting for stage 6 to
// move it to a normal wave instead of traversing here
enum : int { PH_IDLE = 0, PH_TRAV = 1, PH_READY = 2, PH_PARK = 3 };

// kFeat (RT_FEAT_*): the scene features the variant carries code for — instance
// chains (cornell scenes), (u, v)-reading materials (earth()), checker textures
// (the random scenes).  The host launches the smallest compiled variant covering
// the scene (final(): media only); RT_FEAT_ALL runs anything.
// kMode, the closest-hit search:
//   0  BVH in HBM (nodes through L1/L2), 4-wave workgroups, 24-entry LDS stacks;
//   1  BVH2 nodes in LDS (one workgroup of RT_LDS_BLOCK threads per CU copies them
//      at launch; node steps read them with ds_read_b128), stacks of the scene's depth;
//   2  flat scan of the primitive groups (rt_layout.h rt_dgroup), primitives in LDS,
//      no BVH and no stack: scenes of at most RT_SCAN_MAX primitives.
// kMode & 4 (kFold, RT_FLAG_RIGHT_FOLD): the right-fold variants of the plain width-2
// kernels.  A sample's radiance is main.cpp:36's `emitted + attenuation*color(...)`
// evaluated from the deepest hit outwards instead of throughput * emitted: each scatter
// stores its attenuation in the lane's own stack in HBM (RtKernelArgs.fold, depth-major:
// a wave's entries of one depth are contiguous), the path's end folds them back.  The
// lane that writes an entry is the only one that reads it (no ball waves: paths stay in
// their lane), so plain loads and stores in program order suffice.  The switch shares
// the search mode's template argument so that the other variants keep their names.
// kMode & 8 (kRays, rt_kernel_rays.hip): the ray-source variants behind rt_radiance_rays
// (rt_hip.h).  A work item is one caller-supplied ray record (RtKernelArgs.rays,
// 48 B: origin, time, direction, the draws already spent, the stream's pixel and sample
// numbers) instead of a camera sample: refill makes the sample starts from the records (key,
// stream position after the skipped draws, the validity test), the camera stage takes origin,
// direction and time from the record and draws nothing, and a finished item stores its 16 B
// (rgb, status) straight into RtKernelArgs.radiance: no slab, no resolve.  The stages between
// are the shared ones, so a record that restates a camera sample returns that sample's
// radiance bit for bit.  RT_FEAT_ALL, width 2, forward throughput only.
// Kernel arguments re-read each loop iteration: the persistent
// loop reads ~40 uniform arguments; held in SGPRs across it they overflowed the 102
// addressable SGPRs, which the compiler spilled into the lanes of a VGPR (v_writelane
// at entry, a v_readlane — a VALU issue — per use).  Through a kernarg pointer that is
// made opaque at the top of every iteration they are scalar loads (SMEM, scalar
// cache) at their first use in the iteration instead (c4 53.01 -> 52.24 ms, c3
// 45.55 -> 45.44 ms; SGPR spills 36 -> 0).
typedef __attribute__((address_space(4))) const RtKernelArgs KArgs;
__device__ __forceinline__ KArgs *opaque_kargs(KArgs *p) {
    asm volatile("" : "+s"(p));
    return p;
}

// The ray-source variants (kMode & 8) carry every feature's code and, unbounded, allocate
// about 160 VGPRs: at the other variants' 4 waves per SIMD (128 VGPRs) they spilled 6 to 51 of
// them to scratch.  They are built for 3 waves per SIMD (168 VGPRs, no scratch), and their
// BVH2-in-LDS workgroup is 12 waves instead of 16 (a 16-wave workgroup is 4 per SIMD).
#define RT_RAYS_WAVES_PER_SIMD 3
#define RT_RAYS_LDS_BLOCK (RT_RAYS_WAVES_PER_SIMD * 4 * 64)
constexpr int rt_mega_block(int mode) { return (mode & 3) == 1 ? ((mode & 8) ? RT_RAYS_LDS_BLOCK : RT_LDS_BLOCK) : RT_BLOCK; }
constexpr int rt_mega_waves(int mode) { return (mode & 8) ? RT_RAYS_WAVES_PER_SIMD : RT_WAVES_PER_SIMD; }

template <bool kCount, bool kProf, int kWidth, int kFeat, int kMode>
__global__ __launch_bounds__(rt_mega_block(kMode), rt_mega_waves(kMode)) void rt_megakernel(RtKernelArgs A_param) {
    (void)A_param;   // read through ka (the same bytes: the kernarg segment holds A_param at offset 0)
    KArgs *ka = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
#define A (*(const RtKernelArgs *)ka)
    constexpr bool kInst = (kFeat & RT_FEAT_INST) != 0, kUV = (kFeat & RT_FEAT_UV) != 0,
                   kChecker = (kFeat & RT_FEAT_CHECKER) != 0, kPrescan = (kFeat & RT_FEAT_PRESCAN) != 0,
                   kMedia = (kFeat & RT_FEAT_MEDIA) != 0;
    constexpr int kSearch = kMode & 3;
    constexpr bool kFold = (kMode & 4) != 0;
    constexpr bool kRays = (kMode & 8) != 0;
    constexpr bool kLds = kSearch == 1, kScan = kSearch == 2;
    // the ball waves (stage 6) and the medium cell that ends their paths' closest-hit searches
    // (stage 3): the media variant without instance chains (final(); a cell needs a medium
    // bounded by one plain sphere, and the instance variants have no registers to spare) with
    // the BVH2 in LDS.  The cell is tested in ball waves only: in the others, whose lanes
    // mostly start outside the ball, its lockstep tests cost every lane (c4 +3.8 %)
    constexpr bool kBall = kMedia && !kInst && kFeat != RT_FEAT_ALL && kLds && kWidth == 2 && !kFold;
    constexpr bool kCell = kBall;
    // refill finishes the samples of provably empty pixels itself (RtKernelArgs.empty_bits) in the
    // plain width-2 media variant: final()'s, which also runs the scenes with no feature at all.
    // (With the instance chains' code the block spilled, 12 B of scratch per lane in cornell_box's
    // LDS variant; in the random scenes' variant, whose benchmark camera has a lens and never
    // uses it, its mere presence cost c3 1.2 %: profiles/r16.  The other variants ignore the bits,
    // their samples take the generic stages, and their refill is the one they had.)
    constexpr bool kEmptyFast = kFeat == RT_FEAT_MEDIA && kWidth == 2 && !kFold;
    // refill may take items out of the sample starts it makes (kEmptyFast: the samples it finished;
    // kRays: the invalid rays, whose zero record it stores): the survivors are compacted
    constexpr bool kCompact = kEmptyFast || kRays;
    // the LDS node layout (rt_device.h RtSplit): dword planes in the media variants (final()),
    // float4 planes otherwise, as each measured fastest
    constexpr int kSplit = rt_lds_split(kSearch, kFeat, kWidth);
    constexpr int kBlock = rt_mega_block(kMode);
    __shared__ uint32_t lds_stack[kSearch ? 1 : RT_BLOCK / 64][kSearch ? 1 : (kWidth >= 8 ? RT_STACK_DEPTH_W8 : RT_STACK_DEPTH)][64];
    __shared__ CoopSlot lds_slots[kBlock / 64][64];
    __shared__ MediumRec lds_media[RT_LDS_MEDIA];
    __shared__ CamV4 lds_cam[6];
    __shared__ MediaConsts lds_mconst;
    __shared__ U4j lds_jump[RT_LCG_JUMPS];   // drand48 jump-ahead table (coop_reject)
    // per wave: the next RT_PRE work items' sample starts, made 64 at a time (refill)
    __shared__ uint64_t lds_pre_key[kBlock / 64][RT_PRE];
    __shared__ float2 lds_pre_uv[kBlock / 64][RT_PRE];
    __shared__ uint2 lds_pre_cp[kBlock / 64][RT_PRE];   // each entry's (sample chunk, job pixel)
    // stage 6's path pools (kBall): [0] paths inside the ball, [1] paths outside; a lock, the
    // two counts and the number of ball waves still running
    __shared__ U4p lds_pool_in[kBall ? RT_BALL_POOL : 1][5];
    __shared__ U4p lds_pool_out[kBall ? RT_NORM_POOL : 1][5];
    __shared__ uint32_t lds_pool_ctl[4];
    // (kBall) Perlin's tables (perlin.h:76-79: 256 gradients, 3 x 256 permutations), 7 KiB of
    // the LDS the 16-bit stacks left: the noise texture's dependent gathers from LDS
    __shared__ F4v lds_ranvec[kBall ? 256 : 1];
    __shared__ int lds_perm[kBall ? 768 : 1];
    extern __shared__ float4 lds_dyn[];   // kLds: node planes, then the stacks
    const uint32_t lane = lane_id();
    // the wave's index in the workgroup is wave-uniform: its LDS bases live in SGPRs
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (LDS variant: 16-bit entries, [wave][depth][lane], rt_device.h stk16_*)
    uint32_t *stk = kLds ? reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(lds_dyn) + lds_node_bytes<kSplit>() +
                                                        (wave * (uint32_t)A.stack_depth * 64u + lane) * 2u)
                         : &lds_stack[kSearch ? 0 : wave][0][lane];
    CoopSlot *slots = lds_slots[wave];
    uint64_t *pre_key = lds_pre_key[wave];
    float2 *pre_uv = lds_pre_uv[wave];
    uint2 *pre_cp = lds_pre_cp[wave];
    // the media records are read from LDS (one broadcast read per medium)
    if (kMedia) load_media<kBlock>(A, lds_media);
    if (threadIdx.x == 0) {
        lds_pool_ctl[0] = lds_pool_ctl[1] = lds_pool_ctl[2] = 0;
        // (no medium cell: no paths for ball waves, none run)
        lds_pool_ctl[3] = kBall && A.cell_n > 0 ? (uint32_t)min(max(A.ball_waves, 0), kBlock / 64) : 0u;
        store_camera(A, lds_cam);
        lds_mconst = LogConsts{1.0 / 7, -1.0 / 6, 0.2, -0.25, 1.0 / 3};
    }
    for (uint32_t i = threadIdx.x; i < RT_LCG_JUMPS; i += kBlock) lds_jump[i] = kLcgJump.e[i];
    if (kBall) {
        for (uint32_t i = threadIdx.x; i < 256; i += kBlock) {
            const float4 v = A.ranvec[i];
            lds_ranvec[i] = F4v{v.x, v.y, v.z, v.w};
        }
        for (uint32_t i = threadIdx.x; i < 768; i += kBlock) lds_perm[i] = A.perm[i];
    }
    rtl_lds_init(threadIdx.x);   // rt_libm.h's sine constants
    const LdsJump *jt = (const LdsJump *)lds_jump;
    if (kLds) {
        // interior child references become byte offsets into the planes (n * 16): a
        // node step's LDS address is then the reference itself (LdsNodes)
        for (uint32_t i = threadIdx.x; i < A.nnodes; i += kBlock) {
            const float4 *N = A.nodes + i * 4;
            const float4 b0 = N[0], b1 = N[1], b2 = N[2];
            float4 cf = N[3];
            const uint32_t c0 = (uint32_t)fbits(cf.x), c1 = (uint32_t)fbits(cf.y);
            // leaves in the 16-bit stack form (rt_device.h RT_LDS_LEAF16)
            cf.x = __uint_as_float((c0 & RT_LEAF_BIT) ? RT_LDS_LEAF16(c0) : lds_node_ref<kSplit>(c0));
            cf.y = __uint_as_float((c1 & RT_LEAF_BIT) ? RT_LDS_LEAF16(c1) : lds_node_ref<kSplit>(c1));
            if constexpr (kSplit) {   // one dword per node and plane (rt_device.h RtSplit)
                float *P = reinterpret_cast<float *>(lds_dyn) + i;
                constexpr uint32_t C = RT_LDS_NODE_CAP;
                P[RS_C0 * C] = cf.x; P[RS_C1 * C] = cf.y;
                P[RS_XLO * C] = b0.x; P[(RS_XLO + 1) * C] = b1.z; P[RS_XHI * C] = b0.y; P[(RS_XHI + 1) * C] = b1.w;
                P[RS_YLO * C] = b0.z; P[(RS_YLO + 1) * C] = b2.x; P[RS_YHI * C] = b0.w; P[(RS_YHI + 1) * C] = b2.y;
                P[RS_ZLO * C] = b1.x; P[(RS_ZLO + 1) * C] = b2.z; P[RS_ZHI * C] = b1.y; P[(RS_ZHI + 1) * C] = b2.w;
                continue;
            }
            // the references, then per-axis planes (LdsNodes::load_signed): (lo0, hi0, lo1, hi1) of x, y, z
            lds_dyn[i] = cf;
            lds_dyn[i + RT_LDS_NODE_CAP] = make_float4(b0.x, b0.y, b1.z, b1.w);
            lds_dyn[i + 2 * RT_LDS_NODE_CAP] = make_float4(b0.z, b0.w, b2.x, b2.y);
            lds_dyn[i + 3 * RT_LDS_NODE_CAP] = make_float4(b1.x, b1.y, b2.z, b2.w);
        }
    }
    __syncthreads();
    const GlobalNodes gnodes{A.nodes};
    const LdsNodes<kSplit> lnodes{(const LdsF4 *)lds_dyn};

    const uint64_t skey = kRays ? 0 : seed_key(A.seed);   // per-launch part of the sample keys (kRays: made in refill)
    // wave-uniform claim pool, and the pre-made sample starts [pre_head, pre_head + pre_count)
    uint32_t pool_next = 0, pool_end = 0;
    bool exhausted = false;
    // entries [pre_head, pre_head + pre_count) of the wave's pre-made sample starts
    uint32_t pre_head = 0, pre_count = 0;

    // lane state: work item, path, traversal
    uint32_t item = 0xFFFFFFFFu;
    int s_cur = 0, s_end = 0;
    V3 part = mk(0, 0, 0);
    int phase = PH_IDLE;
    bool finished = false;
    Ray r;
    r.o = mk(0, 0, 0); r.d = mk(0, 0, 0); r.time = 0;
    V3 beta = mk(1, 1, 1);
    int depth = 0;
    Rng g; g.x = 0; g.xm = 0;
    // this lane's pre-made sample start, taken by retire_and_claim for camera_begin
    // (read out at once: a refill later in the same claim reuses the slots)
    bool pre_have = false;
    uint64_t pre_k = 0;
    float2 pre_cuv = make_float2(0.f, 0.f);
    uint32_t node = 0;
    int sp = 0;
    float best_t = RT_FLT_MAX;
    int best_key = 0x7FFFFFFF;
    uint32_t best_prim = 0xFFFFFFFFu;

    Counters cnt;
    uint64_t cnt_empty = 0;   // (kCount) samples refill finished itself (rt_stats.empty_fast_samples)
    uint64_t prof[5] = {0, 0, 0, 0, 0};   // claim, traverse, media, shade, of which scatter branches
    uint64_t prof_iters = 0;              // (kProf) this wave's loop iterations
    uint64_t fast_trips = 0, fast_cycles = 0;   // (kProf) the fused in-ball step's trips and their cycles (part of traverse)
    uint64_t stamp = kProf ? __builtin_amdgcn_s_memtime() : 0;
    // wave timeline (kProf): start, first sight of the empty pool, end (s_memrealtime: one clock for all CUs)
    const uint64_t rt_start = kProf ? __builtin_amdgcn_s_memrealtime() : 0;
    uint64_t rt_exhaust = 0;
    uint32_t rt_items = 0;   // work items this wave claimed (kProf)
    uint64_t dr_iters = 0, dr_live = 0, dr_taken = 0;   // (kProf) after the dry point: iterations, live lanes, pooled paths taken
    uint64_t dr_prof[4] = {0, 0, 0, 0};                 // (kProf) ... and the stage cycles (claim, traverse, media, shade)
    auto mark = [&](int k) {
        if (kProf) {
            const uint64_t now = __builtin_amdgcn_s_memtime();
            prof[k] += now - stamp;
            if (exhausted) dr_prof[k < 4 ? k : 3] += now - stamp;
            stamp = now;
        }
    };
    // a new ray segment: closest-hit search from the root (hitable_list.h:20-32)
    bool fresh = false;   // a new segment the pre-scan has not seen yet
    auto begin_segment = [&](bool counted = true) {
        if (kPrescan || kCell) fresh = true;
        // LDS mode: byte offsets (the root is interior there)
        node = kLds ? lds_node_ref<kSplit>(A.root) : A.root;
        sp = 0;
        best_t = RT_FLT_MAX;
        best_key = 0x7FFFFFFF;
        best_prim = 0xFFFFFFFFu;
        phase = A.has_bvh ? PH_TRAV : PH_READY;
        if (kCount && counted) cnt.segments++;
    };

    // Sample starts are made for 64 work items at once, by all lanes of the wave
    // (refill): each item's pixel, sample key, medium-stream key and the two jitter
    // draws (main.cpp:305-306) — four of a new sample's five hashes, which a lane
    // starting a sample alone would run at the few-lane occupancy of path
    // regeneration.  They wait in the wave's LDS slots until a lane takes one.
    auto refill = [&]() {   // all 64 lanes; wave-uniform outcome
        if (pool_next == pool_end) {
            // claims are counted, not items: claim k < nbig covers A.claim items, later
            // ones A.claim_tail (the launch's last items go out in small claims, so that
            // no wave is left with a large claim while the others have run dry)
            uint32_t k = 0;
            if (lane == 0) k = atomicAdd(A.counter, 1u);
            k = __shfl(k, 0);
            const uint32_t big = min(k, A.nbig);
            const uint64_t b64 = (uint64_t)big * A.claim + (uint64_t)(k - big) * A.claim_tail;
            const uint32_t base = (uint32_t)min(b64, (uint64_t)A.nitems);
            const uint32_t size = k < A.nbig ? A.claim : A.claim_tail;
            if (base >= A.nitems) {
                exhausted = true;
                if (kProf) rt_exhaust = __builtin_amdgcn_s_memrealtime();
                return;
            }
            pool_next = base;
            pool_end = min(base + size, A.nitems);
        }
        const uint32_t n = min(64u, pool_end - pool_next);
        if (kProf) rt_items += n;
        const bool mine = lane < n;
        uint32_t c = 0, pj = 0;
        uint64_t K = 0;
        float cu = 0.f, cv = 0.f;
        bool gone = false;
        if constexpr (kRays) {
            // 64 ray records -> 64 sample starts.  The key is the record's own (pixel, sample) under
            // the launch's seed; the main stream restarts there and jumps the record's `skip` draws
            // (one table entry: skip <= RT_LCG_JUMPS - 1); the medium stream's key is derived from K
            // where the sample starts (Rng::start), so it is not affected.  The slots hold (item, -),
            // K and, in pre_uv's 8 bytes, the 48-bit stream position.  An invalid record (rt_hip.h:
            // a non-finite origin, direction or time, a zero direction, a time outside a moving
            // scene's span, a skip past the table) gets its zero record here and leaves the slots.
            static_assert(RT_RADIANCE_MAX_SKIP == RT_LCG_JUMPS - 1, "rt_hip.h states the jump table's reach");
            // (the arguments through a pointer of the block's own, and the seed's key made here: held
            // in SGPRs from the kernel's start they were spilled to a VGPR's lanes)
            KArgs *kb = opaque_kargs(ka);
#define B (*(const RtKernelArgs *)kb)
            if (mine) {
                const uint32_t it = pool_next + lane;
                const float4 q0 = B.rays[(size_t)it * 3 + 0], q1 = B.rays[(size_t)it * 3 + 1], q2 = B.rays[(size_t)it * 3 + 2];
                const uint32_t skip = __float_as_uint(q1.w);
                auto fin = [](float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; };
                const bool ok = fin(q0.x) && fin(q0.y) && fin(q0.z) && fin(q0.w) && fin(q1.x) && fin(q1.y) && fin(q1.z) &&
                                !(q1.x == 0.f && q1.y == 0.f && q1.z == 0.f) && skip <= (uint32_t)RT_RADIANCE_MAX_SKIP &&
                                (!B.rays_moving || (q0.w >= B.rays_t0 && q0.w <= B.rays_t1));
                if (ok) {
                    K = sample_key(seed_key(B.seed), __float_as_uint(q2.x), __float_as_uint(q2.y));
                    const uint64_t x = lcg_jump(K & kLcgM, jt[skip]);
                    pre_cp[lane] = make_uint2(it, 0u);
                    pre_key[lane] = K;
                    pre_uv[lane] = make_float2(__uint_as_float((uint32_t)x), __uint_as_float((uint32_t)(x >> 32)));
                } else {
                    __builtin_nontemporal_store(F4v{0.f, 0.f, 0.f, __int_as_float(RT_HIT_INVALID)}, (F4v *)B.radiance + it);
                    gone = true;
                }
            }
#undef B
        }
        if (!kRays && mine) {
            // item -> (sample chunk c, job pixel p): the job's first ndeep pixels (capi_render.cpp:
            // those whose primary rays enter a dense medium) have all their chunks first,
            // sample-major, then the other pixels' (RtKernelArgs.ndeep)
            const uint32_t it = pool_next + lane;
            if (it < A.ndeep_items) {
                c = it / A.ndeep;
                pj = it - c * A.ndeep;
            } else {
                const uint32_t i2 = it - A.ndeep_items, nb = A.npix - A.ndeep;
                c = i2 / nb;
                pj = A.ndeep + (i2 - c * nb);
            }
            const uint32_t xy = A.job_xy[pj];
            const int x = (int)(xy & 0xFFFFu), j = A.ny - 1 - (int)(xy >> 16);
            // the pixel key in uint32_t: j * nx passes INT_MAX in the upper half of a 65535-wide frame
            K = sample_key(skey, (uint32_t)j * (uint32_t)A.nx + (uint32_t)x, c * (uint32_t)A.chunk + A.sample_offset);
            // main.cpp:305-306; A.rnx = RN(1/float(nx)) from the host (div_rn)
            const uint64_t x1 = lcg_step(K & kLcgM), x2 = lcg_step(x1);   // the sample's first two draws
            cu = div_rn((float)((double)x + u48x(x1)), (float)A.nx, A.rnx);
            cv = div_rn((float)((double)j + u48x(x2)), (float)A.ny, A.rny);
            pre_cp[lane] = make_uint2(c, pj);
            pre_key[lane] = K;
            pre_uv[lane] = make_float2(cu, cv);
        }
        // Samples of provably empty pixels (A.empty_bits, one bit per job pixel: no primary ray of
        // the pixel can reach a surface; empty_pixels.cpp, which also checks that the lens radius
        // is 0, chunk 1 and the rest of what follows relies on) are finished right here.  Such a
        // sample is its camera ray (camera_finish with the zero lens offset: origin and direction
        // are the pinhole's, whatever the disk draw), one medium_one per medium against
        // t_max = FLT_MAX from the sample's own medium stream, and, unless a medium scatters, the
        // miss radiance: the generic stages' own expressions, so images are bitwise unchanged.  A
        // sample a medium scatters stays among the sample starts untouched and is served from
        // scratch by the generic stages, as is one with a zero direction component (there the sign
        // of x - (+-0) depends on the disk draw).  The others' items leave the slots: the survivors
        // are compacted below.  (The item's values wait in the lane's own slot meanwhile: held in
        // registers across the media they spilled.)
        if (kEmptyFast && A.empty_bits != nullptr) {   // wave-uniform
            const bool flagged = mine && ((A.empty_bits[pj >> 5] >> (pj & 31u)) & 1u) != 0u;
            if (wballot(flagged) != 0ull) {
                // (the arguments through a pointer of the block's own, read here: none of them is held
                // in SGPRs from the iteration's start across the media, where they spilled)
                KArgs *kb = opaque_kargs(ka);
#define B (*(const RtKernelArgs *)kb)
                const CamView C = load_camera(lds_cam);
                Ray q;
                q.o = C.org;
                q.d = sub(add(add(C.llc, scale(cu, C.hor)), scale(cv, C.ver)), C.org);
                q.time = C.t0;   // a closed shutter, or no boundary that moves
                const bool el = flagged && q.d.x != 0.f && q.d.y != 0.f && q.d.z != 0.f;
                if (el) {
                    const bool nd = B.need_dlen != 0;
                    const Recip rd = recip_of(nd ? len(q.d) : 0.f, nd);
                    int mm = -1;
                    const uint64_t c_sph = cnt.spheres, c_msp = cnt.mspheres, c_rec = cnt.rects, c_ins = cnt.instanced,
                                   c_med = cnt.media;   // (kCount) a scattered sample is counted by the generic stages alone
                    if constexpr (kMedia) {   // media_hit with nothing found yet
                        const Recip ra = recip_of(dot(q.d, q.d), true);
                        uint64_t xm = mix64(pre_key[lane] ^ 0xD1B54A32D192ED03ull) & kLcgM;   // Rng::start
                        bool have = false;
                        float bt = RT_FLT_MAX;
                        const int nl = min(B.nmedia, RT_LDS_MEDIA);
                        for (int k = 0; k < nl; ++k) {
                            const MediumRec M = lds_medium_rec(lds_media, k);
                            xm = lcg_step(xm);
                            medium_one<kCount, kInst, true>(B, M, k, q, rd, ra, xm, have, bt, mm, (LdsMediaConsts *)&lds_mconst, cnt);
                        }
                        for (int k = RT_LDS_MEDIA; k < B.nmedia; ++k) {
                            MediumRec M;
                            M.md = B.media[k];
                            M.g0 = B.bprims[M.md.x * 4 + 0];
                            M.mm = B.bprims[M.md.x * 4 + 1];
                            xm = lcg_step(xm);
                            medium_one<kCount, kInst, true>(B, M, k, q, rd, ra, xm, have, bt, mm, (LdsMediaConsts *)&lds_mconst, cnt);
                        }
                    }
                    if (mm < 0) {
                        ShadeState st0;
                        st0.kind = -1; st0.live = false; st0.wants_sphere = false; st0.tv = mk(0, 0, 0);
                        // end_path of a first segment: de_nan(1 * e), then 0 + it
                        V3 L = mul(mk(1, 1, 1), shade_emitted(B, false, q, rd, st0));
                        if (!(L.x == L.x)) L.x = 0;
                        if (!(L.y == L.y)) L.y = 0;
                        if (!(L.z == L.z)) L.z = 0;
                        L = add(mk(0, 0, 0), L);
                        const uint2 cp = pre_cp[lane];
                        float *sl = B.slab + ((size_t)cp.x * B.npix + cp.y) * RT_SLAB_FLOATS;
                        sl[0] = L.x;
                        sl[1] = L.y;
                        sl[2] = L.z;
                        gone = true;
                        if (kCount) { cnt.samples++; cnt.segments++; cnt_empty++; }
                    } else if (kCount) {
                        cnt.spheres = c_sph; cnt.mspheres = c_msp; cnt.rects = c_rec; cnt.instanced = c_ins;
                        cnt.media = c_med;
                    }
                }
            }
#undef B
        }
        const uint64_t keep = kCompact ? wballot(mine && !gone) : 0ull;
        if (kCompact && wballot(gone) != 0ull) {   // the survivors move up, in order
            const bool stay = mine && !gone;
            const uint2 cp = pre_cp[lane];
            const uint64_t k = pre_key[lane];
            const float2 uv = pre_uv[lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (stay) {
                const uint32_t e = lanes_below(keep);
                pre_cp[e] = cp;
                pre_key[e] = k;
                pre_uv[e] = uv;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        pre_head = 0;
        pre_count = kCompact ? (uint32_t)__popcll(keep) : n;
        pool_next += n;
    };
    // ---- stage 6's path pools (kBall; DESIGN.md §5c "ball waves") ----------------------
    // The workgroup's last A.ball_waves waves gather the paths whose segment starts inside
    // the medium cell's ball: their closest-hit searches end at the cell's few primitives
    // with no BVH descent, so a wave made of them skips the traversal stage.  Paths move
    // between waves through two LDS pools at segment starts (the whole path state, 80 B:
    // ray, throughput, depth, both drand48 states, the work item and its partial sum), so
    // every sample's draws, adds and slab slot are its own wherever it runs: images are
    // bitwise unchanged.  One spin lock guards both pools; a wave leaves the kernel only
    // after seeing both pools empty, so no path is stranded.
    const bool ballrole = kBall && A.cell_n > 0 && (int)wave >= kBlock / 64 - A.ball_waves;   // wave-uniform
    typedef __attribute__((address_space(3))) volatile uint32_t LdsVU;
    auto pool_peek = [&](int k) -> uint32_t {   // a racy hint; decisions are made under the lock
        return __builtin_amdgcn_readfirstlane(((LdsVU *)lds_pool_ctl)[1 + k]);
    };
    // (A.ball_drain) with the claims exhausted a normal wave leaves the ball's paths to the ball
    // waves while one runs: there the medium cell ends their searches (in a normal wave a ball
    // path's segment took a full descent, in iterations that wait for the slowest lane: 17 us
    // against 11 in the drain, profiles/r06/wave_drain*.json).  A ball wave leaves under the lock
    // and lowers the count there, so a path pushed to the ball's pool after the last one left
    // is seen by its pusher, which takes it back or stays until the pool is empty.
    auto ball_pool_mine = [&]() -> bool {
        return ballrole || !A.ball_drain || __builtin_amdgcn_readfirstlane(((LdsVU *)lds_pool_ctl)[3]) == 0u;
    };
    auto pool_lock = [&]() {
        if (lane == 0)
            while (atomicCAS(&lds_pool_ctl[0], 0u, 1u) != 0u) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    };
    auto pool_unlock = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) atomicExch(&lds_pool_ctl[0], 0u);
    };
    auto pool_entry = [&](int k, uint32_t e) -> U4p * { return k == 0 ? lds_pool_in[e] : lds_pool_out[e]; };
    // lanes with `want` (a fresh segment) leave for pool k while it has room; returns who left
    auto pool_push = [&](int k, bool want) -> bool {
        const uint64_t M = wballot(want);
        if (M == 0ull) return false;
        const uint32_t cap = k == 0 ? RT_BALL_POOL : RT_NORM_POOL;
        // the last ball wave has left: nobody is coming for the ball's pool but the pusher itself
        // (a stale read only sends a path the old way: the pusher stays until the pool is empty)
        if (k == 0 && __builtin_amdgcn_readfirstlane(((LdsVU *)lds_pool_ctl)[3]) == 0u) return false;
        if (pool_peek(k) >= cap) {
            if (kCount && k == 0 && lane == 0) cnt.ball[RT_BALL_DENIED] += (uint64_t)__popcll(M);
            return false;
        }
        pool_lock();
        const uint32_t n = __builtin_amdgcn_readfirstlane(((LdsVU *)lds_pool_ctl)[1 + k]);
        const uint32_t take = min((uint32_t)__popcll(M), cap - min(n, cap));
        const uint32_t rank = lanes_below(M);
        const bool go = want && rank < take;
        if (go) {
            U4p *E = pool_entry(k, n + rank);
            E[0] = U4p{__float_as_uint(r.o.x), __float_as_uint(r.o.y), __float_as_uint(r.o.z), __float_as_uint(r.time)};
            E[1] = U4p{__float_as_uint(r.d.x), __float_as_uint(r.d.y), __float_as_uint(r.d.z), __float_as_uint(beta.x)};
            E[2] = U4p{__float_as_uint(beta.y), __float_as_uint(beta.z), __float_as_uint(part.x), __float_as_uint(part.y)};
            E[3] = U4p{__float_as_uint(part.z), item, (uint32_t)s_cur, (uint32_t)s_end};
            E[4] = U4p{(uint32_t)g.x, (uint32_t)(g.x >> 32) | ((uint32_t)depth << 16), (uint32_t)g.xm, (uint32_t)(g.xm >> 32)};
        }
        if (lane == 0) ((LdsVU *)lds_pool_ctl)[1 + k] = n + take;
        pool_unlock();
        if (kCount && lane == 0) {
            cnt.ball[k == 0 ? RT_BALL_PUSH_IN : RT_BALL_PUSH_OUT] += take;
            if (k == 0) cnt.ball[RT_BALL_DENIED] += (uint64_t)__popcll(M) - take;
        }
        return go;
    };
    // lanes with `need` take paths from pool k (a fresh segment each); returns who took one
    auto pool_take = [&](int k, bool need) -> bool {
        const uint64_t M = wballot(need);
        if (M == 0ull || pool_peek(k) == 0u) return false;
        pool_lock();
        const uint32_t n = __builtin_amdgcn_readfirstlane(((LdsVU *)lds_pool_ctl)[1 + k]);
        const uint32_t take = min((uint32_t)__popcll(M), n);
        const uint32_t rank = lanes_below(M);
        const bool got = need && rank < take;
        if (got) {
            const U4p *E = pool_entry(k, n - take + rank);
            const U4p e0 = E[0], e1 = E[1], e2 = E[2], e3 = E[3], e4 = E[4];
            r.o = mk(__uint_as_float(e0.x), __uint_as_float(e0.y), __uint_as_float(e0.z));
            r.time = __uint_as_float(e0.w);
            r.d = mk(__uint_as_float(e1.x), __uint_as_float(e1.y), __uint_as_float(e1.z));
            beta = mk(__uint_as_float(e1.w), __uint_as_float(e2.x), __uint_as_float(e2.y));
            part = mk(__uint_as_float(e2.z), __uint_as_float(e2.w), __uint_as_float(e3.x));
            item = e3.y;
            s_cur = (int)e3.z;
            s_end = (int)e3.w;
            g.x = ((uint64_t)(e4.y & 0xFFFFu) << 32) | e4.x;
            depth = (int)(e4.y >> 16);
            g.xm = ((uint64_t)e4.w << 32) | e4.z;
        }
        if (lane == 0) ((LdsVU *)lds_pool_ctl)[1 + k] = n - take;
        pool_unlock();
        if (kCount && lane == 0) cnt.ball[RT_BALL_TAKEN] += take;
        if (kProf && exhausted) dr_taken += take;
        if (got) {
            finished = false;
            pre_have = false;
            begin_segment(false);   // (the segment was counted where it began)
        }
        return got;
    };

    // (medium cell) whether the lane's ray starts inside the cell's ball, and if so tsafe: a
    // distance safely below where it leaves the ball (stage 3's cell block and fused step)
    auto cell_exit = [&](float &tsafe) -> bool {
        const V3 oc = sub(r.o, mk(A.cell_c[0], A.cell_c[1], A.cell_c[2]));
        const float a = dot(r.d, r.d), b = dot(oc, r.d), cc = dot(oc, oc) - A.cell_r2;
        if (!(cc < 0.f && a > 0.f)) return false;
        // where the ray leaves the ball: the larger root, without cancellation
        // (approximate square root and reciprocals, ~1 ulp each: a bound, not a result)
        const float q = __builtin_amdgcn_sqrtf(b * b - a * cc);
        const float te = b >= 0.f ? -cc * __builtin_amdgcn_rcpf(b + q) : (q - b) * __builtin_amdgcn_rcpf(a);
        tsafe = te * (1.f - 1.f / 4096);   // below it by far more than its rounding
        return true;
    };

    // retire a finished work item (its sum to the slab), hand the lanes without work
    // the next pre-made sample starts (one global atomic per A.claim items).  top: the call
    // at the top of the iteration, the only one that takes pooled paths (kBall; one inlined
    // copy of the path-state load, where two spilled); in the other, a ball wave whose pool
    // holds paths leaves its idle lanes for the next top
    auto retire_and_claim = [&](bool top) {
        if (phase == PH_IDLE && !finished && item != 0xFFFFFFFFu && s_cur == s_end) {
            if constexpr (kRays) {   // the ray's record: its one sample's radiance (0 + de_nan(L)), status 0
                __builtin_nontemporal_store(F4v{part.x, part.y, part.z, __int_as_float(0)}, (F4v *)A.radiance + item);
            } else {
                float *sl = A.slab + (size_t)item * RT_SLAB_FLOATS;   // 12 B per item
                sl[0] = part.x;
                sl[1] = part.y;
                sl[2] = part.z;
            }
            item = 0xFFFFFFFFu;
        }
        bool need = phase == PH_IDLE && !finished && item == 0xFFFFFFFFu;
        if constexpr (kBall) {
            if (top) {
                // a ball wave takes the ball's paths first, the others the paths that left
                // it; lanes that found no work before (finished) look again: the pools refill
                need = phase == PH_IDLE && item == 0xFFFFFFFFu;
                // pool 0 holds the ball's paths, 1 the others'; with the claims exhausted a
                // wave whose own pool is empty takes from the other
                const bool other = exhausted && pool_peek(ballrole ? 0 : 1) == 0u && ball_pool_mine();
                const int k = (other == ballrole) ? 1 : 0;
                if (pool_take(k, need)) need = false;
            }
            if (ballrole && !exhausted) {
                // a ball wave claims new samples only while fewer than A.ball_claim of its lanes
                // hold a path, and outside the top only with its pool empty (its idle lanes wait
                // for the pool's paths at the next top); lanes left idle have no item.  A wave
                // with no path at all always claims at the top: only a claim finds the pool
                // exhausted, and a wave that never did would never leave the kernel.
                const uint32_t busy = (uint32_t)__popcll(wballot(!(phase == PH_IDLE && item == 0xFFFFFFFFu)));
                if ((!top && pool_peek(0) != 0u) || (busy >= (uint32_t)A.ball_claim && !(top && busy == 0u))) return;
            }
        }
        uint64_t need_mask = wballot(need);
        while (need_mask != 0ull) {
            // (a refill may leave no sample start: a block of empty pixels it finished itself)
            if (pre_count == 0) {
                if constexpr (kCompact) {
                    if (exhausted) break;
                    refill();
                    if (pre_count == 0) continue;   // none left, or all of them finished there: look again
                } else {
                    if (!exhausted) refill();
                    if (pre_count == 0) break;
                }
            }
            const uint32_t rank = lanes_below(need_mask);
            if (need && rank < pre_count) {
                const uint32_t e = pre_head + rank;
                pre_k = pre_key[e];
                pre_cuv = pre_uv[e];
                const uint2 cp = pre_cp[e];
                const uint32_t c = cp.x;
                item = c * A.npix + cp.y;   // the slab slot: [chunk][job pixel]
                pre_have = true;
                need = false;
                s_cur = (int)(c * (uint32_t)A.chunk);
                s_end = min(s_cur + A.chunk, A.ns);
                part = mk(0, 0, 0);
                if constexpr (kRays) {   // the item is the ray, its one sample
                    item = cp.x;
                    s_cur = 0;
                    s_end = 1;
                }
            }
            const uint32_t took = min((uint32_t)__popcll(need_mask), pre_count);
            pre_head += took;
            pre_count -= took;
            need_mask = wballot(need);
        }
        if (need) finished = true;
    };
    // a camera sample (main.cpp:305-308, camera.h:41-56): the sample's stream and
    // jitter, then (after the lens-disk point) the ray
    auto camera_begin = [&](bool starting, float &cu_, float &cv_) {
        if constexpr (kRays) {   // the record's stream, where its skipped draws end (refill); no jitter
            if (starting) {
                g.start(pre_k, kMedia);
                g.x = ((uint64_t)__float_as_uint(pre_cuv.y) << 32) | __float_as_uint(pre_cuv.x);
                pre_have = false;
            }
            return;
        }
        if (starting) {
            if (pre_have) {   // a work item's first sample: made by refill
                g.start(pre_k, kMedia);
                g.skip2();   // the two jitter draws
                cu_ = pre_cuv.x;
                cv_ = pre_cuv.y;
                pre_have = false;
            } else {            // a further sample of a multi-sample work item (chunk > 1)
                const uint32_t c = item / A.npix;
                const uint32_t xy = A.job_xy[item - c * A.npix];
                const int px = (int)(xy & 0xFFFFu), j = A.ny - 1 - (int)(xy >> 16);
                g.start(sample_key(skey, (uint32_t)j * (uint32_t)A.nx + (uint32_t)px, (uint32_t)s_cur + A.sample_offset), kMedia);
                cu_ = div_rn((float)((double)px + g.next()), (float)A.nx, A.rnx);
                cv_ = div_rn((float)((double)j + g.next()), (float)A.ny, A.rny);
            }
        }
    };
    // seg: begin the segment here (else the caller does)
    auto camera_finish = [&](bool starting, float cu_, float cv_, V3 disk, bool seg = true) {
        if constexpr (kRays) {   // the first segment is the record's ray: no lens, no time draw
            if (starting) {
                const float4 q0 = A.rays[(size_t)item * 3 + 0], q1 = A.rays[(size_t)item * 3 + 1];
                r.o = mk(q0.x, q0.y, q0.z);
                r.d = mk(q1.x, q1.y, q1.z);
                r.time = q0.w;
                beta = mk(1, 1, 1);
                depth = 0;
                if (kCount) cnt.samples++;
                if (seg) begin_segment();
            }
            return;
        }
        if (starting) {
            const CamView C = load_camera(lds_cam);
            V3 rd = scale(C.lens, disk);
            V3 offset = add(scale(rd.x, C.cu), scale(rd.y, C.cv));
            // camera.h:54: a closed shutter (t1 - t0 == 0, final() and the Cornell scenes)
            // gives time0 + u*0 = time0 for every draw u, so the draw is consumed unhashed
            const float span = C.t1 - C.t0;
            double u = 0.0;
            if (span != 0.0f) u = g.next(); else g.skip();
            float time = (float)((double)C.t0 + u * (double)span);
            V3 org = C.org;
            V3 dir = sub(sub(add(add(C.llc, scale(cu_, C.hor)), scale(cv_, C.ver)), org), offset);
            r.o = add(org, offset);
            r.d = dir;
            r.time = time;
            if (!kFold) beta = mk(1, 1, 1);
            depth = 0;
            if (kCount) cnt.samples++;
            if (seg) begin_segment();
        }
    };
    // a path's radiance into its work item (de_nan, main.cpp:232-242; col += temp)
    auto end_path = [&](V3 L) {
        if (!(L.x == L.x)) L.x = 0;
        if (!(L.y == L.y)) L.y = 0;
        if (!(L.z == L.z)) L.z = 0;
        part = add(part, L);
        ++s_cur;
        phase = PH_IDLE;
    };

    // (kFold) entry 0 of the lane's attenuation stack.  The address is made where it is
    // used, from arguments re-read there (opaque_kargs) and a lane index the compiler
    // cannot carry: hoisted out of the persistent loop it held two VGPRs and two SGPRs for
    // the whole kernel, which spilled.
    auto fold_base = [&]() -> float4 * {
        KArgs *k = opaque_kargs(ka);
        uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
        asm volatile("" : "+v"(slot));
        return k->fold + slot;
    };
    // (kFold) main.cpp:36 from the deepest hit outwards: L is the path end's own emitted
    // value; every scatter above it returns emitted + attenuation * L, its emitted() the
    // base class's vec3(0,0,0) (material.h:56) — the add stays: 0 + x is not x for x = -0
    auto fold_path = [&](V3 L) -> V3 {
        const float4 *f = fold_base();
        for (int d = depth - 1; d >= 0; --d) {
            const float4 att = f[(size_t)d * A.fold_stride];
            L = add(mk(0, 0, 0), mul(mk(att.x, att.y, att.z), L));
        }
        return L;
    };

    for (;;) {
        // (not in the flat-scan variant: its scan reads the group records right at the
        // iteration's start, and the reload measured slower there, c2 37.63 -> 37.88 ms; its
        // fold variants do reload: holding the arguments in SGPRs across the loop beside
        // fold_base's re-read ones spilled 4 SGPRs in two of them, 0 with the reload, and the
        // mode's speed is no concern)
        if (!kScan || kFold) ka = opaque_kargs(ka);
        // ---- 1. claims and camera samples for lanes without a path --------------
        // (the first iteration, and paths that ended after the shading stage's
        // cooperative rounds: a metal's absorbed reflection; the others start their
        // next sample inside stage 5)
        retire_and_claim(true);
        const uint64_t live = wballot(!finished);
        // (kBall) a wave leaves only with the pools it serves empty: paths another wave left there
        // are taken by the next iteration's retire_and_claim (this one runs with no lane active).
        // A ball wave serves both and decides under the lock (ball_pool_mine)
        if (live == 0ull) {
            if (!kBall) break;
            if ((pool_peek(1) | (ball_pool_mine() ? pool_peek(0) : 0u)) == 0u) {
                if (!ballrole) break;
                pool_lock();
                const bool leave = (pool_peek(0) | pool_peek(1)) == 0u;
                if (leave && lane == 0) ((LdsVU *)lds_pool_ctl)[3] = ((LdsVU *)lds_pool_ctl)[3] - 1u;
                pool_unlock();
                if (leave) break;
            }
        }
        // the pool is dry and few paths are left: the launch's end waits on their latency
        const bool dry = exhausted && __popcll(live) <= RT_DRY_LANES;
        {
            const bool starting = phase == PH_IDLE && !finished && (!kBall || item != 0xFFFFFFFFu);
            float cu_ = (RT_SHADE_LEAN & 8) ? unset_f() : 0.f, cv_ = (RT_SHADE_LEAN & 8) ? unset_f() : 0.f;   // starting lanes only
            camera_begin(starting, cu_, cv_);
            const V3 disk = coop_reject<2, kCount>(!kRays && starting, g, slots, jt, lane, cnt, DiskCand());   // (kRays: no lens)
            camera_finish(starting, cu_, cv_, disk);
        }
        mark(0);
        if (kCount && first_active()) cnt.w_iters++;

        // ---- 3. closest surface hit: BVH traversal rounds --------------------
        // A round = descend until all but RT_DESCEND_TAIL searching lanes hold a
        // leaf, test the leaves.  The
        // wave keeps running rounds for the lanes still searching until
        // RT_READY_BATCH lanes have their hit, then shades that batch: a lane that
        // finished early no longer holds the wave in traversal, and a lane still
        // searching keeps its LDS stack and carries on in the next iteration.
        if constexpr (kScan) {
            // ---- 3'. closest surface hit, flat scan: every lane with a new segment,
            // group by group (box test for all lanes, skipped when none hits; one
            // object-space transform per group), primitive by primitive in lockstep.
            const bool act = phase == PH_TRAV;
            if (wballot(act) != 0ull) {
                // the records through the scalar cache (every lane reads the same one): SGPR
                // operands, no LDS round trip per primitive (an LDS copy: c2 52.58 -> 51.93 ms)
                const ConstF4 *P = (const ConstF4 *)A.prims;
                const ConstF4 *G = (const ConstF4 *)A.groups;
                const Slab sl = make_slab<kSplit>(r, A.tmin);
                ScanBest b{best_t, 0x7FFFFFFF};   // a new segment: nothing found yet
                for (int gi = 0; gi < A.ngroups; ++gi) {
                    const F4v gh = G[3 * gi], bx = G[3 * gi + 1], bz = G[3 * gi + 2];
                    float tn, tf;
                    box_span(sl, F2{bx.x, bx.y}, F2{bx.z, bx.w}, F2{bz.x, bz.y}, b.t, tn, tf);
                    const bool in = act && tn <= tf;
                    if (kCount && act) { cnt.nodes++; if (first_active()) cnt.w_nodes++; }
                    if (wballot(in) == 0ull) continue;
                    const int first = __builtin_amdgcn_readfirstlane(fbits(gh.x));
                    const int kinds = __builtin_amdgcn_readfirstlane(fbits(gh.w));
                    const int nyz = __builtin_amdgcn_readfirstlane(fbits(bz.z));
                    const int inst = __builtin_amdgcn_readfirstlane(fbits(gh.z));
                    Ray ro = r;
                    if (kInst && inst >= 0) ro = to_object_uniform(A.insts, inst, r);
                    scan_group<kCount, kInst>(P, first, kinds, nyz, inst, ro, A.tmin, in, b, cnt);
                }
                best_t = b.t;
                if (b.kp != 0x7FFFFFFF) { best_key = b.kp >> 8; best_prim = (uint32_t)(b.kp & 0xff); }
                if (act) phase = PH_READY;
            }
        } else {
            // the medium cell (scene_lower.cpp): a new segment starting inside the ball tests the
            // primitives near it; a hit before the ray leaves the ball is the closest of
            // all (every other primitive lies outside), and the search ends without a descent
            if (kCell && ballrole && A.cell_n > 0) {
                // The fused in-ball step (A.ball_fast > 0).  Nearly every
                // segment a ball wave holds starts inside the ball, is decided by the cell and
                // scatters at a medium whose material is an isotropic of constant albedo (the
                // host checks that of every medium: scene_lower.cpp ball_fast_media).  For such a
                // segment stages 3-5 reduce to the cell test, the media, the sampler's point and
                // six assignments, so a ball wave runs just that, trip after trip, while at least
                // A.ball_fast of its lanes hold such a segment, with no claim, pool or lock.
                // A lane whose segment turns out otherwise (a cell primitive first, the cell
                // undecided, no scatter) is left as it was, the medium stream included, sits out
                // the further trips and is served from scratch by the generic stages below; so is
                // a lane at the depth cap.  A trip raises the depth of the lanes it serves and
                // retires the others, so the loop ends after at most max_depth + 1 trips.  The
                // expressions are the generic stages' own (lockstep_prims, medium_one,
                // coop_reject_mixed): images are bitwise unchanged.
                if (A.ball_fast > 0) {
                    bool sat_out = false;
                    for (;;) {
                        bool el = fresh && phase == PH_TRAV && !sat_out && depth < A.max_depth;
                        float tsafe = 0.f;
                        if (el) el = cell_exit(tsafe);
                        if (__popcll(wballot(el)) < A.ball_fast) break;
                        const uint64_t t_in = kProf ? __builtin_amdgcn_s_memtime() : 0;
                        // (kCount) a lane that is not served is counted by the generic stages alone
                        const uint64_t c_sph = cnt.spheres, c_msp = cnt.mspheres, c_rec = cnt.rects, c_ins = cnt.instanced,
                                       c_med = cnt.media;
                        // a fresh segment: best_t, best_key, best_prim hold begin_segment()'s values
                        lockstep_prims<kCount, kInst, true>((const ConstF4 *)A.prims, A.cell_first, A.cell_n, A.insts, r, A.tmin,
                                                            el, -1, best_t, best_key, best_prim, cnt);
                        const bool decided = el && best_t < tsafe;
                        uint64_t xm = g.xm;
                        int kh = -1;   // the medium that scatters, if any
                        if (el) {      // stage 4's media_hit over the LDS records (at most 2 media here)
                            const Recip rd = recip_of(len(r.d), true);
                            const Recip ra = recip_of(dot(r.d, r.d), true);
                            bool have = best_prim != 0xFFFFFFFFu;
                            const int nl = min(A.nmedia, 2);
                            for (int k = 0; k < nl; ++k) {
                                const MediumRec M = lds_medium_rec(lds_media, k);
                                xm = lcg_step(xm);
                                int mm = -1;
                                medium_one<kCount, kInst>(A, M, k, r, rd, ra, xm, have, best_t, mm, (LdsMediaConsts *)&lds_mconst, cnt);
                                kh = mm >= 0 ? k : kh;
                            }
                        }
                        const bool commit = decided && kh >= 0;
                        if (kCount) {
                            if (el && !commit) {
                                cnt.spheres = c_sph; cnt.mspheres = c_msp; cnt.rects = c_rec; cnt.instanced = c_ins;
                                cnt.media = c_med;
                            }
                            if (commit) { cnt.shades++; cnt.l_scatter++; }
                            const uint64_t nc = wballot(commit), nd = wballot(el && !commit);
                            if (lane == 0) {
                                cnt.ball[RT_BALL_CELL_BALL] += (uint64_t)__popcll(nc);
                                cnt.ball[RT_BALL_FUSED] += (uint64_t)__popcll(nc);       // lanes this trip served
                                cnt.ball[RT_BALL_DECLINED] += (uint64_t)__popcll(nd);    // ... and left to the generic stages
                            }
                        }
                        // material.h:145-149 with the lane's own rejection loop (all 64 lanes run the rounds)
                        const uint64_t trips0 = cnt.w_rius, local0 = cnt.w_local;   // (kCount)
                        const V3 pt = coop_reject_mixed<kCount>(commit, false, g, slots, jt, lane, cnt, A.coop_local,
                                                                A.coop_local_min);
                        if (kCount && lane == 0) {
                            const uint64_t local = cnt.w_local - local0, rounds = cnt.w_rius - trips0 - local;
                            cnt.sampler[RT_SAMPLER_LOCAL] += local;
                            cnt.sampler[RT_SAMPLER_ROUNDS] += rounds;
                            cnt.sampler[RT_SAMPLER_BALL_LOCAL] += local;
                            cnt.sampler[RT_SAMPLER_BALL_ROUNDS] += rounds;
                        }
                        if (commit) {
                            g.xm = xm;
                            r.o = at(r, best_t);
                            r.d = pt;
                            r.time = 0.0f;
                            beta = mul(beta, kh == 0 ? mk(A.ball_alb[0][0], A.ball_alb[0][1], A.ball_alb[0][2])
                                                     : mk(A.ball_alb[1][0], A.ball_alb[1][1], A.ball_alb[1][2]));
                            ++depth;
                            begin_segment();
                        } else if (el) {
                            sat_out = true;
                            best_t = RT_FLT_MAX;
                            best_key = 0x7FFFFFFF;
                            best_prim = 0xFFFFFFFFu;
                        }
                        if (kProf) {
                            fast_trips++;
                            fast_cycles += __builtin_amdgcn_s_memtime() - t_in;
                        }
                    }
                }
                bool in = false;
                float tsafe = 0.f;
                const bool fr = fresh && phase == PH_TRAV;
                if (fr) in = cell_exit(tsafe);
                if (wballot(in) != 0ull) {
                    lockstep_prims<kCount, kInst, true>((const ConstF4 *)A.prims, A.cell_first, A.cell_n, A.insts, r, A.tmin,
                                                        in, -1, best_t, best_key, best_prim, cnt);
                    if (in && best_t < tsafe) phase = PH_READY;
                    if (kCount) {
                        const uint64_t decided = wballot(in && phase == PH_READY);
                        if (lane == 0) cnt.ball[RT_BALL_CELL_BALL] += (uint64_t)__popcll(decided);
                    }
                }
                // a new segment the cell did not decide waits for stage 6 to leave for a normal
                // wave (A.ball_park): a ball wave's few traversing lanes ran its traversal rounds
                // at a few lanes each.  Not once the claims are exhausted: a ball wave then takes
                // the other pool's paths too, and parking them again could pass a path between
                // the pool and a ball wave forever when no normal wave is left
                if (A.ball_park && !exhausted && fr && phase == PH_TRAV) phase = PH_PARK;
            }
            // pre-scan: the scene's largest primitives (scene_lower.cpp), kept out of the BVH,
            // tested in lockstep by every lane with a new segment before its descent;
            // their hits also shorten best_t, which culls more of the BVH
            if (kPrescan && A.nprescan > 0) {
                const bool fr = fresh && phase == PH_TRAV;
                if (wballot(fr) != 0ull)
                    lockstep_prims<kCount, kInst, true>((const ConstF4 *)A.prims, 0, A.nprescan, A.insts, r, A.tmin, fr, -1,
                                                        best_t, best_key, best_prim, cnt);
            }
            if (kPrescan || kCell) fresh = false;
            if (kCount && ballrole && lane == 0) {
                cnt.ball[RT_BALL_ITERS]++;
                cnt.ball[RT_BALL_LIVE] += (uint64_t)__popcll(live);
            }
            const int batch = ballrole ? A.ball_batch : RT_READY_BATCH;
            for (;;) {
                if (wballot(phase == PH_TRAV) == 0ull) break;
                if (__popcll(wballot(phase == PH_READY)) >= batch) break;
                if (kCount && ballrole && lane == 0) cnt.ball[RT_BALL_ROUNDS]++;
                if (phase == PH_TRAV) {
                    // the slab test needs no exact division: boxes are padded (bvh.cpp)
                    Slab sl = make_slab<kSplit>(r, A.tmin);
                    uint32_t pleaf;
                    if constexpr (kLds && kWidth == 2) lnodes.prepare(sl);
                    if constexpr (kLds)
                        pleaf = descend<kWidth, kCount, kInst ? 1 : RT_DESCEND_STEPS>(lnodes, node, sl, best_t, stk, sp, cnt, dry);
                    else
                        pleaf = descend<kWidth, kCount, kInst ? 1 : RT_DESCEND_STEPS>(gnodes, node, sl, best_t, stk, sp, cnt, dry);
                    if (pleaf != RT_EMPTY_CHILD) {
                        const uint32_t first = kLds ? RT_LDS_LEAF16_FIRST(pleaf) : RT_LEAF_FIRST(pleaf),
                                       nleaf = kLds ? RT_LDS_LEAF16_COUNT(pleaf) : RT_LEAF_COUNT(pleaf);
                        // primitives in pairs: both 32-B heads are fetched before either test
                        for (uint32_t q = 0; q < nleaf; q += 2) {
                            const uint32_t ia = first + q;
                            const bool two = q + 1 < nleaf;
                            const uint32_t ib = two ? ia + 1 : ia;
                            const float4 ga = A.prims[ia * 4 + 0], ma = A.prims[ia * 4 + 1];
                            const float4 gb = A.prims[ib * 4 + 0], mb = A.prims[ib * 4 + 1];
                            auto test_pair = [&](auto kinds) {
                                constexpr int kK = decltype(kinds)::value;
                                int key, kind;
                                float t = prim_t_head<kInst, kK>(ga, ma, A.prims, A.insts, ia, r, A.tmin, key, kind);
                                if (kCount) { cnt.prim(kind); if (first_active()) cnt.w_prims++; }
                                keep_closest(true, t, key, ia, best_t, best_key, best_prim);
                                if (two) {
                                    t = prim_t_head<kInst, kK>(gb, mb, A.prims, A.insts, ib, r, A.tmin, key, kind);
                                    if (kCount) { cnt.prim(kind); if (first_active()) cnt.w_prims++; }
                                    keep_closest(true, t, key, ib, best_t, best_key, best_prim);
                                }
                            };
                            // the kinds the wave tests in this pass: a wave of spheres only or of
                            // rects only runs that kind's test alone (final(): most passes)
                            const bool ra = (fbits(ma.x) & 0xff) > RT_PRIM_MOVING_SPHERE;
                            const bool rb = two && (fbits(mb.x) & 0xff) > RT_PRIM_MOVING_SPHERE;
                            const bool sb = two && !rb;
                            if (wballot(ra || rb) == 0ull) test_pair(std::integral_constant<int, 1>());
                            else if (wballot(!ra || sb) == 0ull) test_pair(std::integral_constant<int, 2>());
                            else test_pair(std::integral_constant<int, 3>());
                        }
                    }
                    if (node == RT_EMPTY_CHILD) phase = PH_READY;   // stack empty too (popped above)
                }
            }
        }
        mark(1);
        // Lanes still searching carry on in the next iteration; the others shade.
        // Stages 4-5 keep the whole wave active (the cooperative sampler needs it).
        const bool ready = phase == PH_READY;

        // ---- 4. media after the surfaces, then the hit record -------------------
        bool have = false;
        // |r.d| once per segment, for the media and the specular materials / sky
        const float dlen = (ready && A.need_dlen) ? len(r.d) : 0.f;
        const Recip rd = recip_of(dlen, ready && A.need_dlen);   // its reciprocal, for div_rn
        Hit hr;   // read only by lanes with a hit (shade_begin / shade_finish guard on `have`)
        if (RT_SHADE_LEAN & 2) {
            hr.p = unset_v3(); hr.n = unset_v3(); hr.u = unset_f(); hr.v = unset_f(); hr.mat = 0;   // the index stays defined
        } else {
            hr.p = mk(0, 0, 0); hr.n = mk(0, 0, 0); hr.u = 0.f; hr.v = 0.f; hr.mat = 0;
        }
        if (ready) {
            have = best_prim != 0xFFFFFFFFu;
            const int med_mat = kMedia ? media_hit<kCount, kInst>(A, lds_media, (LdsMediaConsts *)&lds_mconst, r, rd, g, have,
                                                                  best_t, cnt)
                                       : -1;
            if (med_mat >= 0) {
                hr.p = at(r, best_t);
                hr.n = mk(1, 0, 0);
                hr.mat = med_mat;   // constant_medium.h:41-44 leaves u, v stale; no medium texture reads them
            } else if (have) {
                hr = prim_record<kInst, kUV>(A.prims, A.insts, A.mats, best_prim, r, best_t);
            }
        }

        mark(2);
        // ---- 5. shade (main.cpp:27-45, material.h) ------------------------------
        // Paths that end at this segment whatever the scatter draws (a miss, a light,
        // the depth limit) add their radiance, retire, claim and draw their next camera
        // sample's jitter right here, so that the new samples' lens-disk candidates run
        // in the same cooperative rounds as the scattering lanes' sphere candidates.
        typedef __attribute__((address_space(3))) const F4v LdsRanvec;
        typedef __attribute__((address_space(3))) const int LdsPerm;
        const ShadeState st = kBall ? shade_begin<kCount, kUV, kChecker>(A, ready, have, hr, depth, slots, lane, cnt,
                                                                         (LdsRanvec *)lds_ranvec, (LdsPerm *)lds_perm)
                                    : shade_begin<kCount, kUV, kChecker>(A, ready, have, hr, depth, slots, lane, cnt,
                                                                         A.ranvec, A.perm);
        const bool ends = shade_ends(ready, have, st);
        if (kCount) {   // material divergence: the scatter branches this wave pass runs (shade_finish)
            const bool sc = ready && !ends;
            if (wballot(sc) != 0ull) {
                const int kinds = (wballot(sc && st.kind == RT_MAT_LAMBERTIAN) != 0ull) +
                                  (wballot(sc && st.kind == RT_MAT_METAL) != 0ull) +
                                  (wballot(sc && st.kind == RT_MAT_DIELECTRIC) != 0ull) +
                                  (wballot(sc && st.kind == RT_MAT_ISOTROPIC) != 0ull);
                if (first_active()) { cnt.w_shade++; cnt.w_kinds += (uint64_t)kinds; }
                if (sc) cnt.l_scatter++;
            }
        }
        if (ends) {
            const V3 e = shade_emitted(A, have, r, rd, st);
            if constexpr (kFold) end_path(fold_path(e));
            else end_path(mul(beta, e));
        }
        retire_and_claim(false);
        // (a lane left without work by a ball wave's claim, waiting for the pool, has no item)
        const bool starting = phase == PH_IDLE && !finished && (!kBall || item != 0xFFFFFFFFu);
        float cu_ = (RT_SHADE_LEAN & 8) ? unset_f() : 0.f, cv_ = (RT_SHADE_LEAN & 8) ? unset_f() : 0.f;   // starting lanes only
        camera_begin(starting, cu_, cv_);
        // material.h:41-47 for the scattering lanes, camera.h:6-12 for the new samples
        // (most of a ready batch asks: each lane tries its own first candidates, the rounds serve the rest)
        const uint64_t trips0 = cnt.w_rius, local0 = cnt.w_local;   // (kCount)
        const bool lens = !kRays && starting;   // (kRays: a new sample asks for no lens-disk point)
        const V3 pt = coop_reject_mixed<kCount>(st.wants_sphere || lens, lens, g, slots, jt, lane, cnt,
                                                A.coop_local, A.coop_local_min);
        if (kCount && lane == 0) {   // all 64 lanes are active here: lane 0 holds the wave-level trips
            const uint64_t local = cnt.w_local - local0, rounds = cnt.w_rius - trips0 - local;
            cnt.sampler[RT_SAMPLER_LOCAL] += local;
            cnt.sampler[RT_SAMPLER_ROUNDS] += rounds;
            if (ballrole) {
                cnt.sampler[RT_SAMPLER_BALL_LOCAL] += local;
                cnt.sampler[RT_SAMPLER_BALL_ROUNDS] += rounds;
            }
        }
        mark(3);
        // a scattered path and a new camera sample (disjoint lanes: a lane that started
        // a sample this iteration was idle, not ready) begin their next segment in ONE
        // place: the compiler otherwise materialises the segment state in both divergent
        // branches
        bool seg = false;
        if (ready && !ends) {
            const ShadeOut so = shade_finish(A, ready, have, r, rd, hr, st, pt, g);
            if (so.scattered) {
                // (kFold) depth < max_depth here (ShadeState.live, main.cpp:34): the stack's bound
                if constexpr (kFold)
                    fold_base()[(size_t)depth * A.fold_stride] = make_float4(so.att.x, so.att.y, so.att.z, 0.f);
                else
                    beta = mul(beta, so.att);
                r = so.ray;
                ++depth;
                seg = true;
            } else if constexpr (kFold) {
                end_path(fold_path(so.emitted));
            } else {
                end_path(mul(beta, so.emitted));
            }
        }
        mark(4);
        camera_finish(starting, cu_, cv_, pt, false);
        if (seg || starting) begin_segment();
        // ---- 6. regroup (kBall): a scattered path whose new segment starts inside the
        // medium cell's ball leaves a normal wave for the ball waves' pool, one that starts
        // outside leaves a ball wave for the others' pool (while the pool has room); the
        // lane takes new work at the next claim
        if constexpr (kBall) {
            if (A.ball_waves > 0 && A.cell_n > 0) {
                // inside the ball, and not a ray leaving it from its surface (a refraction out of
                // the glass, a reflection off it): the cell would not decide those
                const V3 oc = sub(r.o, mk(A.cell_c[0], A.cell_c[1], A.cell_c[2]));
                const float o2 = dot(oc, oc);
                const bool inball = o2 < A.cell_r2 && (o2 < A.cell_rin2 || dot(oc, r.d) < 0.f);
                const bool parked = phase == PH_PARK;
                if (pool_push(ballrole ? 1 : 0, (seg && (inball != ballrole)) || parked)) {
                    phase = PH_IDLE;
                    item = 0xFFFFFFFFu;
                } else if (parked) {
                    phase = PH_TRAV;   // the pool is full: it traverses here after all
                }
            }
        }
        mark(3);
        if (kProf) {
            prof_iters++;
            if (exhausted) { dr_iters++; dr_live += (uint64_t)__popcll(live); }
        }
    }
    if (kProf && lane == 0) {
        if (kBall) {   // RT_STAT_BALL in the profile variant: the ball waves' stage cycles and iterations
            if (ballrole) {
                for (int k = 0; k < 4; ++k) atomicAdd(&A.stats[RT_STAT_BALL + k], (unsigned long long)(prof[k] + (k == 3 ? prof[4] : 0)));
                atomicAdd(&A.stats[RT_STAT_BALL + 4], (unsigned long long)prof_iters);
                atomicAdd(&A.stats[RT_STAT_BALL + 6], (unsigned long long)fast_trips);
                atomicAdd(&A.stats[RT_STAT_BALL + 7], (unsigned long long)fast_cycles);
            }
            atomicAdd(&A.stats[RT_STAT_BALL + 5], (unsigned long long)prof_iters);
        }
        // the scatter branches' cycles count in the shade stage too
        for (int k = 0; k < 4; ++k) atomicAdd(&A.stats[RT_STAT_PROF + k], (unsigned long long)(prof[k] + (k == 3 ? prof[4] : 0)));
        atomicAdd(&A.stats[RT_STAT_SHADE + 3], (unsigned long long)prof[4]);
        // minima as maxima of the complement (the slots start at 0)
        const unsigned long long rt_end = __builtin_amdgcn_s_memrealtime();
        unsigned long long *T = A.stats + RT_STAT_TIME;
        atomicMax(&T[0], ~(unsigned long long)rt_start);
        atomicMax(&T[1], ~(unsigned long long)(rt_exhaust ? rt_exhaust : rt_end));
        atomicMax(&T[2], (unsigned long long)(rt_exhaust ? rt_exhaust : rt_end));
        atomicMax(&T[3], ~rt_end);
        atomicMax(&T[4], rt_end);
        // sum of the waves' lifetimes (end - own start: no overflow of absolute clock values
        // summed over ~4,096 waves); the waves of a persistent grid start within µs of T[0]
        atomicAdd(&T[5], rt_end - (unsigned long long)rt_start);
        atomicAdd(&T[6], 1ull);
        if (A.wave_log) {   // HW_ID (cu, simd, wave slot, se) and XCC_ID through s_getreg (reads)
            const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            const uint32_t xcc = __builtin_amdgcn_s_getreg((15 << 11) | 20);
            unsigned long long *W = A.wave_log + RT_WAVE_LOG_WORDS * ((size_t)blockIdx.x * (kBlock / 64) + wave);
            W[0] = rt_start;
            W[1] = rt_exhaust ? rt_exhaust : rt_end;
            W[2] = rt_end;
            W[3] = ((unsigned long long)xcc << 32) | hw;
            W[4] = rt_items;
            W[5] = dr_iters;
            W[6] = dr_live;
            W[7] = dr_taken;
            for (int k = 0; k < 4; ++k) W[8 + k] = dr_prof[k];
        }
    }
    if (kCount) {
        uint64_t w[8] = {cnt.w_iters, cnt.w_nodes, cnt.w_prims, cnt.w_rius, cnt.l_rius, cnt.w_shade, cnt.w_kinds, cnt.l_scatter};
        for (int k = 0; k < 8; ++k) {
            uint64_t x = w[k];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
            if (lane == 0 && x) atomicAdd(&A.stats[k < 5 ? RT_STAT_WAVE + k : RT_STAT_SHADE + (k - 5)], (unsigned long long)x);
        }
    }

    if (kCount && lane == 0)
        for (int k = 0; k < RT_SAMPLER_N; ++k)
            if (cnt.sampler[k]) atomicAdd(&A.stats[RT_STAT_SAMPLER + k], (unsigned long long)cnt.sampler[k]);
    if (kCount && kBall && lane == 0)
        for (int k = 0; k < RT_BALL_N; ++k)
            if (cnt.ball[k]) atomicAdd(&A.stats[RT_STAT_BALL + k], (unsigned long long)cnt.ball[k]);
    if (kCount) {
        uint64_t x = cnt_empty;
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if (lane == 0 && x) atomicAdd(&A.stats[RT_STAT_EMPTY], (unsigned long long)x);
    }
    if (kCount) {
        uint64_t v[RT_CNT_N] = {cnt.samples, cnt.segments, cnt.nodes, cnt.spheres, cnt.mspheres, cnt.rects,
                                cnt.instanced, cnt.media, cnt.shades, cnt.noise};
        for (int k = 0; k < RT_CNT_N; ++k) {
            uint64_t x = v[k];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
            if (lane == 0 && x) atomicAdd(&A.stats[k], (unsigned long long)x);
        }
    }
}

#undef A
}  // namespace
