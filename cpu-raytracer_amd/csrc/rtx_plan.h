// rtx_plan.h — which kernels a render call launches, decided once on the host before anything is queued.
//
// Every traversal kernel produces the same bits, so no parity test can see a level handed to the wrong kernel: only the frame time shows it.
// The rules therefore live here, as one pure function of plain values (PlanInputs -> RenderPlan), with nothing of HIP in them, and
// plan_check.cpp pins them on the CPU (`make plan_check`).  rtx_api.hip gathers the inputs, allocates what the plan wants and runs it; the
// hipGraph key of a call is its plan (plus the scene, the queues, the tile range and the AOV targets): whatever a decision depends on changes
// the plan's bytes.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/rtx.h"
#include "rtx_limits.h"

// Tuning knobs (environment, A/B runs and tests): read ONCE per context in rtx_create, validated and clamped there; a value that does not
// parse or lies outside its range leaves the default in place.  Nothing on the render path calls getenv.
struct Knobs {
    long long slot_budget;       // RTX_SLOT_BUDGET        ray slots per batch of tiles (plan_batch)
    long long item_bytes_max;    // RTX_PK_ITEM_BYTES      upper bound of the split walk's item buffer per context
    int shade_grid;              // RTX_SHADE_GRID         k_shade workgroups per CU
    int lane_from_level;         // RTX_LANE_FROM_LEVEL    per-lane kernels from this level on (-1: the rule in plan_render)
    int lane_from_level_any;     // RTX_LANE_FROM_LEVEL_ANY  the same for shadow rays only (-1: follow the rule)
    int split_items;             // RTX_PK_SPLIT           split shadow-ray walk: 0 = off, else the smallest item chunk
    int resolve_block;           // RTX_RESOLVE_BLOCK      k_resolve workgroup size
    int pk4_order;               // RTX_PK4_ORDER          slot order of the 4-wide records (0: smallest stack need first)
    bool merge_any, no_wide, no_wide_closest, fail_item_alloc, graph; int lpt;
    bool fuse_shade;             // RTX_FUSE_SHADE         the closest-hit packet kernel shades its own hits (0: a k_shade launch per level)
    int update_small_max;        // RTX_UPDATE_SMALL_MAX   rtx_update_instances: scenes up to this many instances take the one-workgroup kernel (0: always the multi-launch path)
    int tex_pass_levels;         // RTX_TEX_PASS_LEVELS    rtx_update_texture: mip levels one launch makes below the level it reads, 1 .. 5 (1: a launch per level)
    bool lone_entry;             // RTX_PK_LONE_ENTRY      packet kernels enter a lone instance straight from the packet set-up (0: the iterator path for every scene)
};

// Two facts about a frame's instances and TLAS that let the packet kernels skip work (rtx_packet.h, pk_enter), decided wherever the host
// writes either:
//   lone        one instance, and the TLAS root is a leaf of count 1 whose slot names instance 0, so the root is the one node a walk can reach
//               (reference-built arrays carry an unused slot at index 1, which no walk looks at: the node COUNT is not asked).  Every ray that
//               passes the root's box enters instance 0 and nothing else, so a packet enters it straight from its set-up (no iterator entry,
//               no tlas_indices / instances chase);
//   copy_class  lone, and the top three rows of the instance's world_inv have the bits of 1.0f on the diagonal and +0.0f or -0.0f everywhere
//               else, the translation column included.  Against xform_pos / xform_dir (rtx_math.h, nothing fused): every other term of a row is
//               then +-0 for finite inputs, so x' = 1 * x + (+-0) is x bit for bit whenever x != 0; a component that is itself +-0 can come out
//               with the other sign of zero, and 1 / +-0 = +-inf is a sign the slab test reads.  So a packet none of whose valid lanes has a zero
//               in o.xyz, d.xyz keeps the world-space ray, and every other packet takes the arithmetic.  Not a memcmp against an identity matrix:
//               the host inverts `world` by cofactors, and an identity input leaves -0.0f in off-diagonal cells.  lone_check.cpp pins both.
struct LoneFacts { bool lone, copy_class; };
static inline LoneFacts plan_lone_facts(int instance_count, const rtx_bvh_node * tlas_nodes, int tlas_node_count, const int32_t * tlas_indices, int tlas_index_count,
                                        const rtx_instance * instances) {
    LoneFacts f = { false, false };
    if (instance_count != 1 || tlas_node_count < 1 || tlas_index_count < 1 || !tlas_nodes || !tlas_indices || !instances) return f;
    if (tlas_nodes[0].count != 1 || tlas_nodes[0].left_or_first != 0 || tlas_indices[0] != 0) return f;      // count: no axis bits either, a leaf of one
    f.lone = true;
    uint32_t bits[12]; memcpy(bits, instances[0].world_inv, sizeof(bits));        // cells[i + 4j]: rows 0 .. 2 are the first twelve
    f.copy_class = true;
    for (int k = 0; k < 12; k++) {
        const bool diagonal = k == 0 || k == 5 || k == 10;
        if (diagonal ? bits[k] != 0x3f800000u : (bits[k] & 0x7fffffffu) != 0u) f.copy_class = false;
    }
    return f;
}

// What the uploaded trees ask of the packet kernels' one stack (plan_stack_limits): unfit_mesh = some mesh exceeds the packet kernels' packed
// entries; dt = TLAS levels (inner depth + 1, 0 without a TLAS); blas_any = the deepest mesh's need in the shadow-ray walk (the 4-wide
// records' bound pk4_need, or inner depth + 2 of the binary walk); blas_shared = twice the deepest mesh's inner depth + 2
struct StackFigures { bool unfit_mesh; int dt, blas_any, blas_shared; };

// can_spawn: some material can spawn a reflection / refraction ray, i.e. has a Ks / Kt that is not all zero
static inline bool plan_can_spawn(const rtx_material * materials, size_t count) {
    for (size_t i = 0; i < count; i++)
        for (int a = 0; a < 3; a++) if (materials[i].reflection[a] != 0.0f || materials[i].transmittance[a] != 0.0f) return true;      // != is true for NaN too: conservative
    return false;
}

// Everything the decisions read, as values
struct PlanInputs {
    uint32_t flags; int views;                       // the call: RTX_RENDER_* bits; tiles, views or rays (RTX_CAM_*, rtx_trace.h)
    int tile_count, batch_tiles; bool tile_major, timing;
    Knobs knobs;
    int instance_count, light_count, bounces;        // the scene
    bool heatmap, can_spawn, all_wide;               // can_spawn: plan_can_spawn of the materials; all_wide: every mesh has 4-wide shadow-ray records
    StackFigures stack;
    int n_cu, pk_blocks_closest, pk_blocks_any;      // the grids
    bool lone, copy_class;                           // plan_lone_facts of the frame state (false after a device-side update)
};

enum : int32_t { CLOSEST_PLAIN, CLOSEST_PLAIN_COUNT, CLOSEST_LANE, CLOSEST_PACKET_STATS, CLOSEST_PACKET, CLOSEST_PACKET_FUSED, CLOSEST_PACKET_FUSED_CULL };
enum : int32_t { SHADE_NONE, SHADE_PLAIN, SHADE_COUNT, SHADE_CULL, SHADE_AOV, SHADE_AOV_COUNT, SHADE_AOV_CULL };      // NONE: the closest-hit kernel shaded its own hits
enum : int32_t { ANY_PLAIN, ANY_PLAIN_COUNT, ANY_LANE, ANY_PACKET_STATS, ANY_PACKET, ANY_PACKET_SPLIT };
// one shadow-ray launch: queued after the k_shade of `after_level`, on the main stream (0) or the shadow-ray stream (1), over levels lo .. hi
// (the plain kernels take lo only); items: a k_items launch over the chunks it filled follows
struct AnyLaunch { int32_t after_level, stream, kernel, lo, hi, items; };

// Trivially copyable, no pointers, always produced from a zeroed object: two plans are the same plan exactly when their bytes are equal
struct RenderPlan {
    uint32_t flags; int32_t views;                   // as given: part of the graph key
    int32_t lane, pk_closest, pstat, cull, aov, serial, plain, heatmap;      // the effective modes (plain: a batch traced by the plain kernels)
    int32_t levels;
    int32_t overlap, merged;
    int32_t lane_from, lane_from_closest;
    int32_t closest[RTX_MAX_LEVELS], shade[RTX_MAX_LEVELS];
    int32_t shade_blocks, stream_blocks, resolve_block, pk_waves_closest, stats_stride;      // grids: k_shade, k_resolve (and its workgroup size), closest-hit packet waves
    int32_t n_any; AnyLaunch any[RTX_MAX_LEVELS];    // the shadow-ray schedule, in queueing order
    int32_t split, item_cap;                         // the split walk is on; the item chunk capacity the call wants (0: none)
    int32_t lpt; uint32_t lpt_n;
    int32_t graph_eligible;
    int32_t lone, copy_class;                        // what the packet kernels are told of the frame's lone instance (both 0 with RTX_PK_LONE_ENTRY=0)
};

// Entries the shared closest-hit walk of a packet can have pending (see plan_stack_limits): one far sibling per inner ancestor in both
// trees (dt in the TLAS, inner depth + 1 in the mesh), at most three parked sign-split entries per tree, the iterator entry
static inline int plan_shared_walk_need(const StackFigures & s) {
    const int tlas_sib = s.dt > 0 ? s.dt : 0, blas_sib = s.blas_shared > 2 ? s.blas_shared / 2 - 1 : 0;
    return tlas_sib + (tlas_sib < 3 ? tlas_sib : 3) + 1 + blas_sib + (blas_sib < 3 ? blas_sib : 3);
}

// What the uploaded trees allow the packet kernels (render calls and ray queries): lane = the call takes the per-lane kernels,
// pk_closest = closest-hit packets may walk shared subtrees together.  Only ever turns lane on and pk_closest off.
static inline void plan_stack_limits(const StackFigures & s, bool & lane, bool & pk_closest) {
    if (s.unfit_mesh) lane = true;      // limits of the packet kernels' packed entries
    // The packet kernels keep ONE 64-entry stack per wave (RTX_PK_STACK) for the TLAS part and the BLAS part of a walk together, where the
    // reference has a stack per BVH (BVH_TRAVERSAL_STACK_SIZE each).  Both depths are known on the host, so the choice is made here, and
    // pk_push's overflow path is taken by no walk these rules let through.  What a walk can have pending, from pk_walk's own rules:
    //   TLAS part   one far sibling per inner node on the path: a leaf of the deepest level (depth dt = inner depth + 1) has dt inner
    //               ancestors, so dt of them; closest-hit rays: one parked sign-split entry per AXIS (the lanes that walk on agree on that
    //               axis for the rest of the subtree, and the parked entry is popped only after it): at most min(3, dt), which the older,
    //               coarser "one per level" of 2 dt + 1 also covers; the iterator entry of the leaf being visited: popped when an instance
    //               is entered and pushed again only while the leaf has instances left, so it lies below the BLAS part exactly where a
    //               leaf holds more than one instance.  The host does not look at the leaves: it always counts 1.
    //   BLAS part   shadow rays: the 4-wide records' bound (pk4_need), or one far sibling per level of the binary walk (inner depth + 2);
    //               closest-hit rays that share the walk (always over the BINARY nodes, whatever records the mesh has): one far sibling per
    //               inner ancestor of a deepest leaf, inner depth + 1 = blas_shared / 2 - 1, and again at most min(3, that) parked entries
    //               — the lanes enter the instance with the signs of their model-space directions, which the TLAS part did not sort.
    // The shared closest-hit walk is not only the RTX_RENDER_PACKET_CLOSEST mode.  In the default mode the packets of level 0 share the top of
    // a BLAS walk until few lanes want a node (pk_defer_t0_primary), and a packet with a lane whose inverse direction is not finite, and every
    // packet of an RTX_RENDER_PACKET_STATS call, walks ALL of it together at every level (pk_walk<.., ASM = false>: no lane turns private).  So
    // the third bound below is on the call, not on a threshold: measured on an MI355X before it existed, 31 instances in a chain over a
    // 35-triangle chain (each tree legal for the reference, the rule of the shadow-ray walk satisfied; 67 entries in a replay of the walk, 71
    // by this count) ended in RTX_ERR_LIMIT in the default mode, and 31 over 33 (65 in the replay) in the statistics mode.
    // Scenes beyond a bound (e.g. a chain-shaped TLAS of 60 instances) are traced by the per-lane kernels: a lane of those keeps far
    // siblings only, nothing parked and no iterator entry, but also on ONE stack (RTX_MAX_STACK = 64 entries, k_trace_fast) for both trees:
    // dt + (a leaf's instances - 1) + (inner depth + 1) entries.  Two trees that each fit the reference's per-BVH stack can exceed
    // that together (32 instances in a chain over a 41-triangle chain: 31 + 40); such a frame still ends in RTX_ERR_LIMIT from
    // rtx_get_stats, from every kernel there is.
    if (s.dt + 1 + s.blas_any > RTX_PK_STACK || 2 * s.dt + 1 > RTX_PK_STACK) lane = true;
    if (2 * s.dt + 1 + s.blas_shared > RTX_PK_STACK) pk_closest = false;
    if (plan_shared_walk_need(s) > RTX_PK_STACK) lane = true;
}

// Grids of the streaming kernels (k_shade, k_resolve: grid-stride loops, any grid is correct) follow the batch: level d of a batch of P
// primary slots is given room for P / 2^d rays — the dispatcher spends ~16 ns per workgroup, which is most of a small launch's
// time (a 1/8 tile shard's k_shade launches of levels 1-3: 18 us each with 1 024 workgroups for 74 k / 6 k / 1 k rays).
#define PLAN_LEVEL_BLOCKS_MIN 64      // never fewer workgroups than this, whatever `full` is: stats_stride (plan_render) allows for it
static inline int plan_level_blocks(int primary_slots, int level, int full) {
    const long long want = (((long long)primary_slots >> level) + 255) / 256;
    const long long most = (long long)full < want ? (long long)full : want;
    return (int)(most > PLAN_LEVEL_BLOCKS_MIN ? most : PLAN_LEVEL_BLOCKS_MIN);
}

// Partial tallies level `level`'s shading pass leaves for k_resolve: one per wave of the fused packet kernel, or one per k_shade workgroup
static inline int plan_stats_n(const RenderPlan & p, int primary_slots, int level) {
    return p.shade[level] == SHADE_NONE ? p.pk_waves_closest : plan_level_blocks(primary_slots, level, p.shade_blocks);
}

// one launch_any of the schedule: levels lo .. lane_from-1 by packets, the rest per lane
static inline void plan_add_any(RenderPlan & p, bool packets, int after_level, int stream, int lo, int hi) {
    const bool count_work = (p.flags & RTX_RENDER_COUNT_WORK) != 0, simple = (p.flags & RTX_RENDER_SIMPLE_TRACE) != 0;
    const int packet_kernel = p.split ? ANY_PACKET_SPLIT : ANY_PACKET;
    if (packets && hi >= p.lane_from) {
        if (lo < p.lane_from) p.any[p.n_any++] = AnyLaunch{ after_level, stream, packet_kernel, lo, p.lane_from - 1, p.split };
        p.any[p.n_any++] = AnyLaunch{ after_level, stream, ANY_LANE, lo > p.lane_from ? lo : p.lane_from, hi, 0 };
        return;
    }
    const int kernel = count_work ? ANY_PLAIN_COUNT : simple ? ANY_PLAIN : p.lane ? ANY_LANE : p.pstat ? ANY_PACKET_STATS : packet_kernel;
    p.any[p.n_any++] = AnyLaunch{ after_level, stream, kernel, lo, hi, packets ? p.split : 0 };
}

// The item buffer could not be allocated: the call continues with the non-split packet kernel and no k_items launches.  Nothing else
// changes: lane_from keeps what the split KNOB made it.
static inline void plan_drop_split(RenderPlan & p) {
    p.split = 0; p.item_cap = 0;
    for (int i = 0; i < p.n_any; i++) { if (p.any[i].kernel == ANY_PACKET_SPLIT) p.any[i].kernel = ANY_PACKET; p.any[i].items = 0; }
}

static inline RenderPlan plan_render(const PlanInputs & in) {
    RenderPlan p; memset(&p, 0, sizeof(p));
    const Knobs & K = in.knobs;
    p.flags = in.flags; p.views = in.views;
    p.lone = K.lone_entry && in.lone; p.copy_class = p.lone && in.copy_class;
    const bool count_work = (in.flags & RTX_RENDER_COUNT_WORK) != 0;
    const bool simple = (in.flags & RTX_RENDER_SIMPLE_TRACE) != 0;
    p.cull = (in.flags & RTX_RENDER_CULL_DEAD_SHADOW_RAYS) != 0 && !simple && !count_work;
    bool lane = (in.flags & RTX_RENDER_LANE_TRACE) != 0;
    bool pk_closest = (in.flags & RTX_RENDER_PACKET_CLOSEST) != 0;            // closest-hit packets walk shared subtrees together (default: lanes turn private at once)
    plan_stack_limits(in.stack, lane, pk_closest);
    p.lane = lane; p.pk_closest = pk_closest;
    p.pstat = (in.flags & RTX_RENDER_PACKET_STATS) != 0 && !simple && !count_work && !lane;
    // RTX_RENDER_AOV: level 0 takes k_shade<.., AOV = true> with the bound channels' targets
    p.aov = (in.flags & RTX_RENDER_AOV) != 0;
    p.serial = (in.flags & RTX_RENDER_SERIAL) != 0;
    p.heatmap = in.heatmap; p.plain = count_work || simple || in.heatmap;
    // traversal kernels: packet walk (production), per-lane pair fetch (RTX_RENDER_LANE_TRACE), plain pop-and-test (SIMPLE / COUNT_WORK)
    const bool packets = !count_work && !simple && !lane && !p.pstat;
    // Levels that can hold rays: a hit spawns a reflection / refraction ray only where its material's Ks / Kt is not all zero (Raytracer.cpp:204-213,
    // rtx_shade.h reflection_mask / refraction_mask).  With no such material uploaded the levels >= 1 are provably empty, and their
    // launches — three per level, each a floor of 7-9 us — are not queued (BASELINE configs[1]: diffuse Monkey.obj with NUMBER_OF_BOUNCES 3).
    p.levels = in.can_spawn ? in.bounces + 1 : 1;
    p.stream_blocks = in.n_cu * 8;          // k_resolve (256 threads)
    p.resolve_block = K.resolve_block;
    p.shade_blocks = in.n_cu * K.shade_grid;      // k_shade (RTX_SHADE_BLOCK = 256 threads, 3 resident blocks per CU at 168 VGPRs)
    p.pk_waves_closest = in.pk_blocks_closest * (RTX_PK_BLOCK / RTX_WAVE);
    p.stats_stride = p.shade_blocks > p.pk_waves_closest ? p.shade_blocks : p.pk_waves_closest;      // per level: one entry per k_shade workgroup, or per wave of the fused packet kernel
    // a k_shade launch has plan_level_blocks' floor of workgroups even where shade_blocks is smaller (few CUs, RTX_GRID_CUS): each writes its entry
    if (p.stats_stride < PLAN_LEVEL_BLOCKS_MIN) p.stats_stride = PLAN_LEVEL_BLOCKS_MIN;

    // Item chunks of the split shadow-ray walk (rtx_packet.h, k_items): one chunk per wave of the packet launch, sized ONCE per call for its
    // largest batch — ≈0.3 items per shadow ray in the cfg3 frame, the fullest chunk 3x the average, so 3.5x the expected average, in
    // whole units of 64 items.  The buffer only ever grows, never beyond knobs.item_bytes_max (1 GiB; a chunk that fills up merely makes the
    // packet keep its nodes, which the kernel supports), and only before anything of the call is queued.  If the allocation
    // fails the pending HIP error is cleared and the call continues with the non-split kernel (plan_drop_split): a correctly queued frame
    // must not report RTX_ERR_HIP.  The split walk needs 4-wide records for every mesh.
    if (K.split_items > 0 && in.light_count > 0 && in.all_wide) {
        const size_t chunks = (size_t)in.pk_blocks_any * (RTX_PK_BLOCK / RTX_WAVE);
        const double expect = 0.45 * 1024.0 * (double)in.batch_tiles * in.light_count / (double)chunks;
        long long cap = K.split_items;
        if (cap < (long long)(3.5 * expect)) cap = ((long long)(3.5 * expect) + 63) & ~63ll;
        const long long cap_max = (K.item_bytes_max / (long long)(chunks * 48)) & ~63ll;
        if (cap > cap_max) cap = cap_max;
        if (cap > (1 << 16)) cap = 1 << 16;
        if (cap >= 64) { p.split = 1; p.item_cap = (int32_t)cap; }
    }

    // RTX_PK_LPT: the level-0 closest-hit launch takes its packets longest first, by what the same packets cost in the previous call of this context
    // over the same tiles (costs written by the launch itself, sorted by k_packet_order on a side stream while the rest of the frame runs).
    // Measured (cfg3): the launch 309 -> 223 us alone, one frame at a time 1.48 -> 1.41 ms; with three frames in flight the tail it removes was
    // being filled by the other frames' kernels anyway (1.090 -> 1.098 ms), and a launch with one packet per wave has nothing to reorder: so by default only
    // in the two-stream shape and with at least two packets per wave.
    p.lpt_n = (uint32_t)in.tile_count * 16u;
    const bool lpt_want = K.lpt > 0 || (K.lpt < 0 && !p.serial && p.lpt_n >= 2u * (uint32_t)p.pk_waves_closest);
    p.lpt = lpt_want && !K.graph && in.tile_count <= in.batch_tiles && packets && !in.heatmap && !K.fuse_shade;
    // hipGraph replay: only for single-batch calls without per-kernel timing
    p.graph_eligible = K.graph && !in.timing && in.tile_count <= in.batch_tiles;

    // Main stream: closest(d) -> shade(d) for d = 0..D.  Shadow rays depend only on shade, so in the default (fast)
    // configuration they run on a second stream: any(level 0) starts after shade(0) and overlaps the deeper levels'
    // closest/shade kernels; the shadow rays of levels 1..D are traced by ONE more launch after shade(D).  This removes
    // three of the per-launch tails (a persistent trace launch has a ~0.17 ms floor set by its slowest rays).
    p.overlap = !count_work && !simple && in.light_count > 0 && !p.serial;
    p.merged = !p.overlap && !count_work && !simple && K.merge_any;

    // Which kernel for which level: a packet's walk of the TLAS costs the UNION of its rays' instances, each entered with its own
    // transform and per-lane phase, so for the incoherent rays of the deeper levels of a multi-instance scene the per-lane kernels
    // (refill, per-lane TLAS walk) win by 2.5-4x (cfg5: closest-hit levels 2 / 3 0.43 / 0.45 -> 0.16 / 0.12 ms, shadow rays 0.41 / 0.35 ->
    // 0.19 / 0.14 ms) while the packet kernels win everywhere else (tools/perlevel3.py).  Both produce the same bits.
    // With hundreds of instances the closest-hit reflection rays of level 1 already prefer the per-lane kernel (tools/many_instances.py:
    // 144 instances 0.52 vs 0.40 ms, 576 instances 0.70 vs 0.39 ms), the shadow rays of level 1 do not (0.48 vs 0.8 ms).
    p.lane_from = K.lane_from_level >= 0 ? K.lane_from_level : (in.instance_count > 1 ? 2 : RTX_MAX_LEVELS + 1);
    p.lane_from_closest = K.lane_from_level >= 0 ? K.lane_from_level : (in.instance_count > 64 ? 1 : p.lane_from);
    // With the split walk a shadow-ray packet that enters an instance with few lanes hands the whole visit over as items, and ONE packet
    // launch for all levels beats a packet launch + a per-lane launch at every instance count measured (tools/any_rule.sh: 16 / 144 / 576
    // instances 1.54 / 2.24 / 3.01 vs 1.66 / 2.41 / 3.05 ms per frame, cfg5 2.32 vs 2.42): shadow rays then stay with the packets.
    // The test is of the split KNOB, not of whether the call got its item buffer.
    if (K.lane_from_level < 0 && K.split_items > 0 && in.light_count > 0 && in.all_wide) p.lane_from = RTX_MAX_LEVELS + 1;
    if (K.lane_from_level_any >= 0) p.lane_from = K.lane_from_level_any;      // shadow rays only (A/B runs)

    // BVH_VISUALIZE_HEATMAP: bounce() returns right after the primary ray's trace (Raytracer.cpp:97-102), so a frame is one
    // closest-hit pass in reference pop order (the plain kernel counts the steps) and one colouring pass
    if (in.heatmap) { p.closest[0] = count_work ? CLOSEST_PLAIN_COUNT : CLOSEST_PLAIN; return p; }

    // Which levels shade their own hits inside the closest-hit packet kernel (k_packet<.., FUSE>, rtx_packet.h) and which get a k_shade
    // launch (every other closest-hit kernel: per-lane, plain, instrumented).  Decided before anything is launched: k_resolve is told
    // how many partial tallies each level's shading pass leaves (plan_stats_n).  The bound is lane_from_closest, not lane_from.
    // Level 0 of an AOV call always has its k_shade launch: the fused packet kernel has no AOV variant (its VGPR budget is tight).
    for (int level = 0; level < p.levels; level++) {
        const bool fused = K.fuse_shade && packets && level < p.lane_from_closest && !(p.aov && level == 0);
        p.closest[level] = count_work ? CLOSEST_PLAIN_COUNT : simple ? CLOSEST_PLAIN : (lane || (!p.pstat && level >= p.lane_from_closest)) ? CLOSEST_LANE :
                           p.pstat ? CLOSEST_PACKET_STATS : fused ? (p.cull ? CLOSEST_PACKET_FUSED_CULL : CLOSEST_PACKET_FUSED) : CLOSEST_PACKET;
        const bool aov0 = p.aov && level == 0;
        p.shade[level] = fused ? SHADE_NONE : count_work ? (aov0 ? SHADE_AOV_COUNT : SHADE_COUNT) : p.cull ? (aov0 ? SHADE_AOV_CULL : SHADE_CULL) : (aov0 ? SHADE_AOV : SHADE_PLAIN);
    }
    if (in.light_count > 0) for (int level = 0; level < p.levels; level++) {
        if (p.overlap) {
            if (level == 0) plan_add_any(p, packets, 0, 1, 0, 0);
            if (level == p.levels - 1 && p.levels > 1) plan_add_any(p, packets, level, 1, 1, p.levels - 1);
        } else if (p.merged) {
            // shadow rays only feed k_resolve: all levels' shadow rays are traced by ONE launch after the last shade
            if (level == p.levels - 1) plan_add_any(p, packets, level, 0, 0, p.levels - 1);
        } else plan_add_any(p, packets, level, 0, level, level);
    }
    return p;
}
