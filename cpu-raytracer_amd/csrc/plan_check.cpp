// plan_check.cpp — the launch plan of rtx_plan.h on the CPU: `make plan_check` builds this with -fsanitize=address,undefined and runs it.
// Every traversal kernel produces the same bits, so which kernel a level is handed to shows in no image: the rules and their measured
// thresholds are pinned here, as named cases of (inputs -> the plan fields that matter).  Needs no GPU and no ROCm.
#include <stdio.h>
#include <initializer_list>
#include <type_traits>
#include "rtx_plan.h"

static_assert(std::is_trivially_copyable<RenderPlan>::value, "the graph key compares a plan's bytes");

static int failures = 0;
static const char * current = "";
#define CASE(name) current = name
#define CHECK(x) do { if (!(x)) { printf("FAILED [%s] line %d: %s\n", current, __LINE__, #x); failures++; } } while (0)

enum { CW = RTX_RENDER_COUNT_WORK, SIMPLE = RTX_RENDER_SIMPLE_TRACE, CULL = RTX_RENDER_CULL_DEAD_SHADOW_RAYS, SERIAL = RTX_RENDER_SERIAL,
       LANE = RTX_RENDER_LANE_TRACE, PSTAT = RTX_RENDER_PACKET_STATS, PKC = RTX_RENDER_PACKET_CLOSEST, AOV = RTX_RENDER_AOV };
static const int NEVER = RTX_MAX_LEVELS + 1;      // a lane_from past every level

// the default frame: one instance, two lights, NUMBER_OF_BOUNCES 3, a reflective material, every mesh with 4-wide records, a 64-tile frame in one batch
static PlanInputs frame() {
    PlanInputs in; memset(&in, 0, sizeof(in));
    in.tile_count = 64; in.batch_tiles = 64;
    Knobs & K = in.knobs;
    K.slot_budget = 48ll * 1000 * 1000; K.item_bytes_max = 1ll << 30; K.shade_grid = 4; K.lane_from_level = -1; K.lane_from_level_any = -1;
    K.split_items = 256; K.resolve_block = 256; K.pk4_order = 1; K.merge_any = true; K.lpt = -1;
    in.instance_count = 1; in.light_count = 2; in.bounces = 3; in.can_spawn = true; in.all_wide = true;
    in.stack = StackFigures{ false, 1, 10, 20 };
    in.n_cu = 256; in.pk_blocks_closest = 1024; in.pk_blocks_any = 1280;
    return in;
}
static PlanInputs frame(uint32_t flags) { PlanInputs in = frame(); in.flags = flags; return in; }

static bool all_closest(const RenderPlan & p, int kernel) { for (int l = 0; l < p.levels; l++) if (p.closest[l] != kernel) return false; return true; }
static bool all_shade(const RenderPlan & p, int kernel) { for (int l = 0; l < p.levels; l++) if (p.shade[l] != kernel) return false; return true; }
static bool same(const RenderPlan & a, const RenderPlan & b) { return memcmp(&a, &b, sizeof(a)) == 0; }
// the shadow-ray schedule as { after_level, stream, kernel, lo, hi, items } rows
static bool schedule(const RenderPlan & p, std::initializer_list<AnyLaunch> want) {
    if (p.n_any != (int)want.size()) return false;
    int i = 0;
    for (const AnyLaunch & w : want) { if (memcmp(&p.any[i], &w, sizeof(w)) != 0) return false; i++; }
    return true;
}

static void modes_and_schedule() {
    CASE("default frame");
    {
        const RenderPlan p = plan_render(frame());
        CHECK(p.levels == 4 && p.overlap && !p.merged && !p.lane && !p.pstat && !p.cull && !p.plain && !p.heatmap);
        CHECK(all_closest(p, CLOSEST_PACKET) && all_shade(p, SHADE_PLAIN));
        CHECK(p.lane_from == NEVER && p.lane_from_closest == NEVER && p.split && p.item_cap == 256);
        CHECK(schedule(p, { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 }, { 3, 1, ANY_PACKET_SPLIT, 1, 3, 1 } }));
        CHECK(p.shade_blocks == 1024 && p.stream_blocks == 2048 && p.resolve_block == 256 && p.pk_waves_closest == 1024 && p.stats_stride == 1024);
        CHECK(plan_stats_n(p, 64 * 1024, 0) == 256 && plan_stats_n(p, 64 * 1024, 3) == 64 && plan_level_blocks(1 << 30, 0, 1024) == 1024);
        const RenderPlan again = plan_render(frame());
        CHECK(same(p, again));                                        // padding included: a plan starts as zeroes
    }
    CASE("instance counts and the split");
    for (int split = 0; split <= 1; split++) {
        const struct { int n, any, closest; } rule[] = { { 2, 2, 2 }, { 64, 2, 2 }, { 65, 2, 1 } };
        for (const auto & r : rule) {
            PlanInputs in = frame(); in.instance_count = r.n; if (!split) in.knobs.split_items = 0;
            const RenderPlan p = plan_render(in);
            CHECK(p.lane_from_closest == r.closest && p.lane_from == (split ? NEVER : r.any) && p.split == split);
            for (int l = 0; l < p.levels; l++) CHECK(p.closest[l] == (l >= r.closest ? CLOSEST_LANE : CLOSEST_PACKET));
            if (split) CHECK(schedule(p, { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 }, { 3, 1, ANY_PACKET_SPLIT, 1, 3, 1 } }));      // shadow rays stay with the packets
            else       CHECK(schedule(p, { { 0, 1, ANY_PACKET, 0, 0, 0 }, { 3, 1, ANY_PACKET, 1, 1, 0 }, { 3, 1, ANY_LANE, 2, 3, 0 } }));
        }
    }
    CASE("split knob on, buffer not had");
    {   // lane_from follows the KNOB: losing the item buffer changes the kernels of the schedule and nothing else
        PlanInputs in = frame(); in.instance_count = 16;
        RenderPlan p = plan_render(in);
        plan_drop_split(p);
        CHECK(!p.split && p.item_cap == 0 && p.lane_from == NEVER && p.lane_from_closest == 2);
        CHECK(schedule(p, { { 0, 1, ANY_PACKET, 0, 0, 0 }, { 3, 1, ANY_PACKET, 1, 3, 0 } }));
        in.all_wide = false;                                              // a mesh without 4-wide records: no split, and the rule of the instance count holds
        p = plan_render(in);
        CHECK(!p.split && p.lane_from == 2);
    }
    CASE("RTX_LANE_FROM_LEVEL");
    for (int v : { 0, 1, 2, 99 }) {
        PlanInputs in = frame(); in.instance_count = 100; in.knobs.lane_from_level = v;
        const RenderPlan p = plan_render(in);
        CHECK(p.lane_from == v && p.lane_from_closest == v);              // both rules and the split's raise are overridden
        for (int l = 0; l < p.levels; l++) CHECK(p.closest[l] == (l >= v ? CLOSEST_LANE : CLOSEST_PACKET));
        if (v == 0)  CHECK(schedule(p, { { 0, 1, ANY_LANE, 0, 0, 0 }, { 3, 1, ANY_LANE, 1, 3, 0 } }));
        if (v == 1)  CHECK(schedule(p, { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 }, { 3, 1, ANY_LANE, 1, 3, 0 } }));
        if (v == 2)  CHECK(schedule(p, { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 }, { 3, 1, ANY_PACKET_SPLIT, 1, 1, 1 }, { 3, 1, ANY_LANE, 2, 3, 0 } }));
        if (v == 99) CHECK(schedule(p, { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 }, { 3, 1, ANY_PACKET_SPLIT, 1, 3, 1 } }));
    }
    CASE("RTX_LANE_FROM_LEVEL_ANY");
    for (int v : { 0, 1, 99 }) {
        PlanInputs in = frame(); in.instance_count = 100; in.knobs.lane_from_level_any = v;
        const RenderPlan p = plan_render(in);
        CHECK(p.lane_from == v && p.lane_from_closest == 1);              // shadow rays only: closest hits keep their rule
        in.knobs.lane_from_level = 3;
        const RenderPlan p2 = plan_render(in);
        CHECK(p2.lane_from == v && p2.lane_from_closest == 3);
    }
    CASE("no material spawns rays");
    {
        PlanInputs in = frame(); in.can_spawn = false;
        for (int b : { 0, 3, 11 }) {
            in.bounces = b;
            const RenderPlan p = plan_render(in);
            CHECK(p.levels == 1 && schedule(p, { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 } }));
        }
        in.can_spawn = true; in.bounces = 11;
        CHECK(plan_render(in).levels == RTX_MAX_LEVELS);
        rtx_material m[2]; memset(m, 0, sizeof(m));
        CHECK(!plan_can_spawn(m, 2) && !plan_can_spawn(m, 0));
        m[1].transmittance[2] = -0.0f; CHECK(!plan_can_spawn(m, 2));
        m[1].transmittance[2] = 1e-30f; CHECK(plan_can_spawn(m, 2));
        m[1].transmittance[2] = 0.0f; m[0].reflection[1] = __builtin_nanf(""); CHECK(plan_can_spawn(m, 2));      // NaN counts as non-zero: conservative
    }
    CASE("no lights");
    {
        PlanInputs in = frame(); in.light_count = 0;
        const RenderPlan p = plan_render(in);
        CHECK(p.n_any == 0 && !p.overlap && !p.split && p.item_cap == 0 && p.merged);
        in.flags = SERIAL;
        CHECK(plan_render(in).n_any == 0);
    }
    CASE("serial");
    {
        PlanInputs in = frame(SERIAL);
        RenderPlan p = plan_render(in);
        CHECK(p.serial && !p.overlap && p.merged && schedule(p, { { 3, 0, ANY_PACKET_SPLIT, 0, 3, 1 } }));
        in.knobs.merge_any = false;
        p = plan_render(in);
        CHECK(!p.merged && schedule(p, { { 0, 0, ANY_PACKET_SPLIT, 0, 0, 1 }, { 1, 0, ANY_PACKET_SPLIT, 1, 1, 1 }, { 2, 0, ANY_PACKET_SPLIT, 2, 2, 1 }, { 3, 0, ANY_PACKET_SPLIT, 3, 3, 1 } }));
        in.knobs.split_items = 0; in.instance_count = 16;                 // a level at or past lane_from is one per-lane launch
        p = plan_render(in);
        CHECK(schedule(p, { { 0, 0, ANY_PACKET, 0, 0, 0 }, { 1, 0, ANY_PACKET, 1, 1, 0 }, { 2, 0, ANY_LANE, 2, 2, 0 }, { 3, 0, ANY_LANE, 3, 3, 0 } }));
        in.knobs.merge_any = true;
        p = plan_render(in);
        CHECK(schedule(p, { { 3, 0, ANY_PACKET, 0, 1, 0 }, { 3, 0, ANY_LANE, 2, 3, 0 } }));
    }
}

static void instrumented_modes() {
    CASE("COUNT_WORK");
    for (uint32_t extra : { 0u, (uint32_t)CULL, (uint32_t)PSTAT, (uint32_t)LANE, (uint32_t)(CULL | PSTAT | SIMPLE) }) {
        const RenderPlan p = plan_render(frame(CW | extra));
        CHECK(p.plain && !p.cull && !p.pstat && !p.overlap && !p.merged && !p.lpt);
        CHECK(all_closest(p, CLOSEST_PLAIN_COUNT) && all_shade(p, SHADE_COUNT));
        CHECK(schedule(p, { { 0, 0, ANY_PLAIN_COUNT, 0, 0, 0 }, { 1, 0, ANY_PLAIN_COUNT, 1, 1, 0 }, { 2, 0, ANY_PLAIN_COUNT, 2, 2, 0 }, { 3, 0, ANY_PLAIN_COUNT, 3, 3, 0 } }));
    }
    CASE("SIMPLE_TRACE");
    for (uint32_t extra : { 0u, (uint32_t)CULL, (uint32_t)PSTAT, (uint32_t)LANE }) {
        const RenderPlan p = plan_render(frame(SIMPLE | extra));
        CHECK(p.plain && !p.cull && !p.pstat && !p.overlap && !p.merged);
        CHECK(all_closest(p, CLOSEST_PLAIN) && all_shade(p, SHADE_PLAIN));
        CHECK(schedule(p, { { 0, 0, ANY_PLAIN, 0, 0, 0 }, { 1, 0, ANY_PLAIN, 1, 1, 0 }, { 2, 0, ANY_PLAIN, 2, 2, 0 }, { 3, 0, ANY_PLAIN, 3, 3, 0 } }));
    }
    CASE("LANE_TRACE");
    for (uint32_t extra : { 0u, (uint32_t)PSTAT }) {                      // pstat is dropped under lane
        const RenderPlan p = plan_render(frame(LANE | extra));
        CHECK(p.lane && !p.pstat && !p.plain && p.overlap && all_closest(p, CLOSEST_LANE) && all_shade(p, SHADE_PLAIN));
        CHECK(schedule(p, { { 0, 1, ANY_LANE, 0, 0, 0 }, { 3, 1, ANY_LANE, 1, 3, 0 } }));
    }
    CASE("LANE_TRACE with CULL");
    {
        const RenderPlan p = plan_render(frame(LANE | CULL | SERIAL));
        CHECK(p.cull && all_shade(p, SHADE_CULL) && schedule(p, { { 3, 0, ANY_LANE, 0, 3, 0 } }));
    }
    CASE("PACKET_STATS");
    {
        PlanInputs in = frame(PSTAT); in.instance_count = 100;            // the instrumented packet kernel at every level, whatever lane_from says
        RenderPlan p = plan_render(in);
        CHECK(p.pstat && all_closest(p, CLOSEST_PACKET_STATS) && all_shade(p, SHADE_PLAIN) && !p.lpt);
        CHECK(schedule(p, { { 0, 1, ANY_PACKET_STATS, 0, 0, 0 }, { 3, 1, ANY_PACKET_STATS, 1, 3, 0 } }));
        in.flags = PSTAT | CULL | SERIAL;
        p = plan_render(in);
        CHECK(p.pstat && p.cull && all_shade(p, SHADE_CULL) && schedule(p, { { 3, 0, ANY_PACKET_STATS, 0, 3, 0 } }));
    }
    CASE("CULL alone");
    {
        const RenderPlan p = plan_render(frame(CULL));
        CHECK(p.cull && all_closest(p, CLOSEST_PACKET) && all_shade(p, SHADE_CULL));
    }
    CASE("fuse_shade");
    {
        PlanInputs in = frame(); in.knobs.fuse_shade = true;
        RenderPlan p = plan_render(in);
        CHECK(all_closest(p, CLOSEST_PACKET_FUSED) && all_shade(p, SHADE_NONE) && !p.lpt && plan_stats_n(p, 64 * 1024, 2) == p.pk_waves_closest);
        in.flags = CULL;
        p = plan_render(in);
        CHECK(all_closest(p, CLOSEST_PACKET_FUSED_CULL) && all_shade(p, SHADE_NONE));
        in.flags = AOV | CULL;                                            // level 0 of an AOV call is never fused
        p = plan_render(in);
        CHECK(p.aov && p.closest[0] == CLOSEST_PACKET && p.shade[0] == SHADE_AOV_CULL);
        for (int l = 1; l < p.levels; l++) CHECK(p.closest[l] == CLOSEST_PACKET_FUSED_CULL && p.shade[l] == SHADE_NONE);
        in.flags = 0; in.instance_count = 65;                            // lane_from_closest = 1 bounds the fused levels; lane_from (past every level) does not
        p = plan_render(in);
        CHECK(p.lane_from_closest == 1 && p.lane_from == NEVER && p.closest[0] == CLOSEST_PACKET_FUSED && p.shade[0] == SHADE_NONE);
        for (int l = 1; l < p.levels; l++) CHECK(p.closest[l] == CLOSEST_LANE && p.shade[l] == SHADE_PLAIN);
        for (uint32_t f : { (uint32_t)CW, (uint32_t)SIMPLE, (uint32_t)LANE, (uint32_t)PSTAT }) {      // only the production packet kernel fuses
            in.flags = f;
            p = plan_render(in);
            for (int l = 0; l < p.levels; l++) CHECK(p.shade[l] != SHADE_NONE);
        }
    }
    CASE("AOV");
    {
        RenderPlan p = plan_render(frame(AOV));
        CHECK(p.shade[0] == SHADE_AOV && p.shade[1] == SHADE_PLAIN);
        p = plan_render(frame(AOV | CW));
        CHECK(p.shade[0] == SHADE_AOV_COUNT && p.shade[1] == SHADE_COUNT);
    }
    CASE("heat map");
    {
        PlanInputs in = frame(); in.heatmap = true;
        RenderPlan p = plan_render(in);
        CHECK(p.heatmap && p.plain && p.closest[0] == CLOSEST_PLAIN && p.n_any == 0 && !p.lpt);
        in.flags = CW;
        p = plan_render(in);
        CHECK(p.closest[0] == CLOSEST_PLAIN_COUNT && p.n_any == 0);
    }
}

static void stack_limits() {
    CASE("stack limits");
    const int S = RTX_PK_STACK;
    auto limits = [](int dt, int blas_any, int blas_shared, bool unfit, bool & lane, bool & pkc) { lane = false; pkc = true; plan_stack_limits(StackFigures{ unfit, dt, blas_any, blas_shared }, lane, pkc); };
    bool lane, pkc;
    limits(10, S - 11, 0, false, lane, pkc); CHECK(!lane && pkc);          // dt + 1 + blas_any == RTX_PK_STACK
    limits(10, S - 10, 0, false, lane, pkc); CHECK(lane && pkc);
    limits((S - 1) / 2, 0, 0, false, lane, pkc); CHECK(!lane);              // 2 dt + 1 == RTX_PK_STACK - 1 (odd): the last depth that fits
    limits((S - 1) / 2 + 1, 0, 0, false, lane, pkc); CHECK(lane);
    limits(10, 0, S - 21, false, lane, pkc); CHECK(!lane && pkc);          // 2 dt + 1 + blas_shared == RTX_PK_STACK
    limits(10, 0, S - 20, false, lane, pkc); CHECK(!lane && !pkc);
    limits(1, 1, 1, true, lane, pkc); CHECK(lane && pkc);                   // a mesh beyond the packed entries
    lane = true; pkc = false; plan_stack_limits(StackFigures{ false, 1, 1, 1 }, lane, pkc); CHECK(lane && !pkc);      // never turns lane off or pk_closest on
    {   // in a plan: lane and pk_closest move separately, and a depth across a bound is a different plan (the graph-key property)
        PlanInputs in = frame(PKC); in.stack = StackFigures{ false, 10, S - 11, S - 21 };
        const RenderPlan fits = plan_render(in);
        CHECK(!fits.lane && fits.pk_closest && all_closest(fits, CLOSEST_PACKET));
        in.stack.blas_shared++;
        const RenderPlan shared_over = plan_render(in);
        CHECK(!shared_over.lane && !shared_over.pk_closest && !same(fits, shared_over));
        in.stack.blas_shared--; in.stack.blas_any++;
        const RenderPlan any_over = plan_render(in);
        CHECK(any_over.lane && any_over.pk_closest && all_closest(any_over, CLOSEST_LANE) && !same(fits, any_over));
        PlanInputs a = frame(), b = frame(); a.stack = StackFigures{ false, (S - 1) / 2, 0, 0 }; b.stack = a.stack; b.stack.dt++;
        CHECK(!same(plan_render(a), plan_render(b)));
        a.flags = b.flags = LANE | PSTAT;                                 // pstat yields to a lane the trees forced, too
        CHECK(!plan_render(b).pstat);
    }
}

// Both trees deep: n instances under a chain-shaped TLAS (dt = n - 1 levels), each a mesh of m triangles under a chain-shaped BVH (inner depth
// m - 2).  blas_any is m for the binary shadow-ray walk and at most RTX_PK4_MAX_NEED - 4 = 32 where the mesh has 4-wide records; blas_shared =
// 2 m.  The combinations are those of tests/stackset.py's grid (c = dt + 1 + blas_any of the binary walk = n + m), whose routing
// tests/test_gpu_packet_stack.py asserts on the device.  The shared closest-hit walk can have (n - 1) + 3 + 1 + (m - 1) + 3 = c + 5 entries
// pending (far siblings of dt = n - 1 and m - 1 inner ancestors, three parks per tree, the iterator entry), so for two chains the third bound
// is the one that binds: c <= 59 packets, beyond it the per-lane kernels.
static void two_deep_trees() {
    CASE("two deep trees");
    const int S = RTX_PK_STACK;
    struct Out { bool lane, pkc; };
    auto rule = [](int n, int m, int blas_any) { Out o = { false, true }; plan_stack_limits(StackFigures{ false, n - 1, blas_any, 2 * m }, o.lane, o.pkc); return o; };
    const struct { int c, n; } grid[] = { { 58, 31 }, { 58, 21 }, { 58, 8 }, { 61, 31 }, { 61, 22 }, { 61, 8 }, { 63, 31 }, { 63, 23 }, { 63, 8 }, { 64, 31 }, { 64, 24 }, { 64, 8 },
                                          { 65, 31 }, { 65, 24 }, { 65, 8 }, { 66, 31 }, { 66, 25 }, { 66, 9 } };
    for (const auto & g : grid) {
        const int n = g.n, m = g.c - g.n;
        CHECK(plan_shared_walk_need(StackFigures{ false, n - 1, m, 2 * m }) == g.c + 5);
        const Out binary = rule(n, m, m), wide = rule(n, m, m < 32 ? m : 32);      // RTX_PK_WIDE=0, and 4-wide records: the shadow-ray walk needs less
        CHECK(binary.lane == (g.c + 5 > S) && wide.lane == binary.lane);     // the shared walk is over the binary nodes whatever the records
        CHECK(!binary.pkc && !wide.pkc);                                    // 2 dt + 1 + 2 m is far beyond the stack everywhere on the grid
    }
    CHECK(!rule(31, 28, 28).lane && rule(31, 29, 29).lane);               // c + 5 = 64 / 65, TLAS-heavy
    CHECK(!rule(8, 51, 32).lane && rule(8, 52, 32).lane);                 // the same, mesh-heavy
    {   // the deepest TLAS leaf holds two instances: the iterator entry then really lies below the BLAS part.  31 instances under a chain of
        // dt = 29 levels over a 29- / 30-triangle chain: 29 + 3 + 1 + 28 + 3 = 64 (packets), 29 + 3 + 1 + 29 + 3 = 65 (per lane); the rule counts
        // the entry whatever the leaves hold, so 30 single-instance leaves (dt = 29) route the same way
        bool lane = false, pkc = true;
        CHECK(plan_shared_walk_need(StackFigures{ false, 29, 29, 58 }) == 64 && plan_shared_walk_need(StackFigures{ false, 29, 30, 60 }) == 65);
        plan_stack_limits(StackFigures{ false, 29, 29, 58 }, lane, pkc); CHECK(!lane);
        plan_stack_limits(StackFigures{ false, 29, 30, 60 }, lane, pkc); CHECK(lane);
        CHECK(plan_shared_walk_need(StackFigures{ false, 2, 4, 8 }) == 2 + 2 + 1 + 3 + 3);      // small trees: parks are bounded by the siblings
        CHECK(plan_shared_walk_need(StackFigures{ false, 0, 2, 4 }) == 0 + 0 + 1 + 1 + 1);
    }
    CHECK(!rule(32, 4, 3).lane && rule(33, 4, 3).lane);                   // 2 dt + 1 = 63 / 65 over a shallow mesh: the older bound still decides there
    CHECK(!rule(1, 60, 59).lane && !rule(1, 61, 32).lane && rule(1, 62, 32).lane);      // one instance: 1 + (m - 1) + 3; the 60-triangle chain of the unit tests stays with the packets
    CHECK(!rule(1, 1, 1).lane && !rule(2, 2, 2).lane);                    // trees of one leaf
    {   // the shadow-ray bound alone (dt + 1 + blas_any = 64 / 65): a mesh whose 4-wide records need more than its binary depth
        bool lane = false, pkc = true;
        plan_stack_limits(StackFigures{ false, 31, 32, 2 * 22 }, lane, pkc); CHECK(!lane);      // shared walk: 31 + 3 + 1 + 21 + 3 = 59
        lane = false; plan_stack_limits(StackFigures{ false, 31, 33, 2 * 22 }, lane, pkc); CHECK(lane);
    }
    {   // the deepest trees among the golden scenes and the benchmark's (TLAS inner depth, deepest mesh's inner depth): cube (-1, 4), monkey (-1, 11),
        // materials / dynamic (1, 11), tori16 (3, 11), the atrium (-1, 24).  All far inside every bound: their plans are what they were
        const struct { int dt, depth; } shipped[] = { { 0, 4 }, { 0, 11 }, { 2, 11 }, { 4, 11 }, { 0, 24 } };
        for (const auto & t : shipped) {
            bool lane = false, pkc = true;
            const StackFigures f = { false, t.dt, t.depth + 2, 2 * (t.depth + 2) };
            plan_stack_limits(f, lane, pkc);
            CHECK(!lane && pkc && plan_shared_walk_need(f) <= 32);
        }
    }
    {   // in a plan: a depth across the bound is a different plan (and a different graph key): lane, the kernels of every level, the shadow-ray schedule
        PlanInputs a = frame(), b = frame();
        a.instance_count = b.instance_count = 31;
        a.stack = StackFigures{ false, 30, 28, 56 }; b.stack = StackFigures{ false, 30, 29, 58 };
        RenderPlan pa = plan_render(a), pb = plan_render(b);
        CHECK(!pa.lane && pb.lane && !same(pa, pb) && all_closest(pb, CLOSEST_LANE) && pa.closest[0] == CLOSEST_PACKET);
        CHECK(schedule(pb, { { 0, 1, ANY_LANE, 0, 0, 0 }, { 3, 1, ANY_LANE, 1, 3, 0 } }));
        a.flags = b.flags = PKC | PSTAT;                                  // the flag is dropped on both sides, silently; the statistics mode yields to the forced lane
        pa = plan_render(a); pb = plan_render(b);
        CHECK(!pa.pk_closest && !pb.pk_closest && pa.pstat && !pb.pstat);
    }
}

static void lpt_items_graph() {
    CASE("LPT");
    {
        PlanInputs in = frame(); in.tile_count = 4; in.pk_blocks_closest = 32;      // 64 packets over 32 waves: two per wave
        RenderPlan p = plan_render(in);
        CHECK(p.lpt && p.lpt_n == 64);
        in.pk_blocks_closest = 33;
        CHECK(!plan_render(in).lpt);
        in.pk_blocks_closest = 32;
        PlanInputs off = in; off.flags = SERIAL;          CHECK(!plan_render(off).lpt);
        off = in; off.knobs.graph = true;                   CHECK(!plan_render(off).lpt);
        off = in; off.batch_tiles = 3;                      CHECK(!plan_render(off).lpt);
        off = in; off.flags = CW;                           CHECK(!plan_render(off).lpt);
        off = in; off.flags = SIMPLE;                       CHECK(!plan_render(off).lpt);
        off = in; off.flags = LANE;                         CHECK(!plan_render(off).lpt);
        off = in; off.flags = PSTAT;                        CHECK(!plan_render(off).lpt);
        off = in; off.heatmap = true;                       CHECK(!plan_render(off).lpt);
        off = in; off.knobs.fuse_shade = true;              CHECK(!plan_render(off).lpt);
        off = in; off.stack.unfit_mesh = true;              CHECK(!plan_render(off).lpt);
        off = in; off.knobs.lpt = 0;                        CHECK(!plan_render(off).lpt);
        PlanInputs on = in; on.knobs.lpt = 1; on.flags = SERIAL; on.pk_blocks_closest = 1024;
        CHECK(plan_render(on).lpt);                                       // 1: whatever the shape
        on.knobs.graph = true;
        CHECK(!plan_render(on).lpt);                                      // but never in a graph call
    }
    CASE("item capacity");
    {
        PlanInputs in = frame();                                          // 1 280 chunks; expected average 0.45 * 1024 * tiles * lights / chunks
        CHECK(plan_render(in).item_cap == 256);                           // 3.5 x 46 items: the floor at the knob's value
        in.knobs.split_items = 64;
        CHECK(plan_render(in).item_cap == 192);                           // 161 rounded up to whole units of 64
        in = frame(); in.batch_tiles = 200; in.tile_count = 200;
        CHECK(plan_render(in).item_cap == 512);                           // 3.5 x 144 = 504
        in.knobs.item_bytes_max = 1280ll * 48 * 128;
        CHECK(plan_render(in).item_cap == 128 && plan_render(in).split);  // the cap by item_bytes_max wins over the floor
        in.knobs.item_bytes_max = 1280ll * 48 * 63;
        const RenderPlan none = plan_render(in);
        CHECK(none.item_cap == 0 && !none.split && none.lane_from == NEVER);      // below 64: no split (lane_from still follows the knob)
        CHECK(schedule(none, { { 0, 1, ANY_PACKET, 0, 0, 0 }, { 3, 1, ANY_PACKET, 1, 3, 0 } }));
        in = frame(); in.batch_tiles = 100000; in.tile_count = 100000; in.light_count = 4; in.knobs.item_bytes_max = 1ll << 36;
        CHECK(plan_render(in).item_cap == 1 << 16);
    }
    CASE("graph");
    {
        PlanInputs in = frame(); in.knobs.graph = true;
        CHECK(plan_render(in).graph_eligible);
        in.timing = true;  CHECK(!plan_render(in).graph_eligible);
        in.timing = false; in.knobs.graph = false; CHECK(!plan_render(in).graph_eligible);
    }
    CASE("more tiles than a batch");
    {
        PlanInputs in = frame(); in.knobs.graph = true; in.knobs.lpt = 1; in.tile_count = 65;
        RenderPlan p = plan_render(in);
        CHECK(!p.graph_eligible && !p.lpt);
        in.knobs.graph = false;
        p = plan_render(in);
        CHECK(!p.graph_eligible && !p.lpt);
        in.tile_count = 64;
        CHECK(plan_render(in).lpt);
    }
    CASE("the key sees flags and views");
    {
        PlanInputs a = frame(), b = frame(); b.views = 1;      // a view call (RTX_CAM_VIEWS)
        CHECK(!same(plan_render(a), plan_render(b)));
        b = frame(CULL);
        CHECK(!same(plan_render(a), plan_render(b)));
    }
}

// Grids of a device with very few compute units (or RTX_GRID_CUS): n_cu 1, 2 and 8 with 8 to 32 one-wave packet workgroups, the 60 tiles of a
// 320 x 180 frame.  shade_blocks = 4 n_cu is then below the floor of plan_level_blocks, which a k_shade launch has all the same.
static void small_grids() {
    const struct { int n_cu, pk_closest, pk_any; } grids[] = { { 1, 8, 8 }, { 1, 16, 8 }, { 2, 16, 24 }, { 2, 32, 32 }, { 8, 32, 32 }, { 8, 8, 16 } };
    auto small = [](int n_cu, int pkc, int pka, uint32_t flags) {
        PlanInputs in = frame(flags); in.n_cu = n_cu; in.pk_blocks_closest = pkc; in.pk_blocks_any = pka; in.tile_count = in.batch_tiles = 60;
        return in;
    };
    CASE("small grids: a level's partial tallies fit its stride");
    for (const auto & g : grids)
        for (int fuse = 0; fuse <= 1; fuse++)
            for (uint32_t flags : { 0u, (uint32_t)SERIAL, (uint32_t)LANE, (uint32_t)CW, (uint32_t)SIMPLE, (uint32_t)AOV, (uint32_t)(CULL | SERIAL) }) {
                PlanInputs in = small(g.n_cu, g.pk_closest, g.pk_any, flags); in.knobs.fuse_shade = fuse != 0; in.bounces = RTX_MAX_LEVELS - 1;
                for (int shade_grid : { 1, 4, 64 }) {
                    in.knobs.shade_grid = shade_grid;
                    const RenderPlan p = plan_render(in);
                    CHECK(p.levels == RTX_MAX_LEVELS && p.shade_blocks == g.n_cu * shade_grid && p.pk_waves_closest == g.pk_closest);
                    CHECK(p.stats_stride >= 64 && p.stats_stride >= p.shade_blocks && p.stats_stride >= p.pk_waves_closest);
                    for (int slots : { 1024, 60 * 1024, 2025 * 1024 })
                        for (int l = 0; l < p.levels; l++) {
                            const int n = plan_stats_n(p, slots, l);
                            CHECK(n >= 1 && n <= p.stats_stride);          // entry level * stride + n - 1 stays inside the level's own stride
                            CHECK(n == (p.shade[l] == SHADE_NONE ? g.pk_closest : plan_level_blocks(slots, l, p.shade_blocks)));
                        }
                    if (fuse && flags == 0u) CHECK(all_shade(p, SHADE_NONE));      // the fused shape was among them
                    if (!fuse) for (int l = 0; l < p.levels; l++) CHECK(p.shade[l] != SHADE_NONE);
                }
            }
    {   // one compute unit, four k_shade workgroups wanted: 64 are launched, and level 11's last entry is (11 * stride + 63) of (12 + 1) * stride
        const RenderPlan p = plan_render(small(1, 8, 8, 0u));
        CHECK(p.shade_blocks == 4 && p.stats_stride == 64 && plan_stats_n(p, 60 * 1024, 0) == 64 && plan_stats_n(p, 60 * 1024, 3) == 64);
        CHECK(plan_render(small(8, 32, 32, 0u)).stats_stride == 64 && plan_render(small(32, 96, 96, 0u)).stats_stride == 128);
        CHECK(plan_render(frame()).stats_stride == 1024);                 // the full device: as before
    }
    CASE("small grids: item capacity follows the chunk count");
    {   // expected average 0.45 * 1024 * 60 tiles * 2 lights / chunks, 3.5 x that in whole units of 64
        CHECK(plan_render(small(1, 8, 8, 0u)).item_cap == 24192);         // 8 chunks: 3.5 x 6 912
        CHECK(plan_render(small(2, 16, 16, 0u)).item_cap == 12096);       // 16 chunks: 3.5 x 3 456
        CHECK(plan_render(small(8, 32, 32, 0u)).item_cap == 6080);        // 32 chunks: 3.5 x 1 728 = 6 048, rounded up
        PlanInputs in = small(1, 8, 8, 0u); in.tile_count = in.batch_tiles = 200;
        CHECK(plan_render(in).item_cap == 1 << 16 && plan_render(in).split);      // 3.5 x 23 040 = 80 640: clipped
        in.knobs.item_bytes_max = 8ll * 48 * 128;
        CHECK(plan_render(in).item_cap == 128 && plan_render(in).split);  // the buffer's bound wins
        in.knobs.item_bytes_max = 8ll * 48 * 63;
        CHECK(plan_render(in).item_cap == 0 && !plan_render(in).split);
        in = small(1, 8, 8, 0u); in.knobs.split_items = 64; in.tile_count = in.batch_tiles = 1; in.light_count = 1;
        CHECK(plan_render(in).item_cap == 256);                           // one tile, one light: 3.5 x 57.6 = 201, in whole units
    }
    CASE("small grids: the LPT default rule");
    for (const auto & g : grids) {
        PlanInputs in = small(g.n_cu, g.pk_closest, g.pk_any, 0u);      // 960 packets over at most 32 waves
        RenderPlan p = plan_render(in);
        CHECK(p.lpt && p.lpt_n == 960);
        in.flags = SERIAL;
        CHECK(!plan_render(in).lpt);
        in.knobs.lpt = 1;
        CHECK(plan_render(in).lpt);
        in.flags = 0; in.knobs.lpt = 0;
        CHECK(!plan_render(in).lpt);
        in.knobs.lpt = -1; in.tile_count = in.batch_tiles = g.pk_closest / 8;      // exactly two packets per wave, and one tile less
        CHECK(plan_render(in).lpt);
        if (g.pk_closest > 8) { in.tile_count = in.batch_tiles = g.pk_closest / 8 - 1; CHECK(!plan_render(in).lpt); }
    }
}

// The plan at the limit: RTX_MAX_LEVELS levels (bounces 11), for every combination of the call's flags and of the knobs a level index enters.
// Whatever the combination, the per-level arrays are filled for all 12 levels and for no more, the shadow-ray schedule fits its array
// and covers every level exactly once, and nothing is queued after a level that does not exist.
static void twelve_levels() {
    CASE("twelve levels");
    const int L = RTX_MAX_LEVELS;
    static_assert(sizeof(((RenderPlan *)0)->any) / sizeof(AnyLaunch) == RTX_MAX_LEVELS && sizeof(((RenderPlan *)0)->closest) / sizeof(int32_t) == RTX_MAX_LEVELS &&
                  sizeof(((RenderPlan *)0)->shade) / sizeof(int32_t) == RTX_MAX_LEVELS, "the plan's per-level arrays");
    long plans = 0;
    for (uint32_t bits = 0; bits < 256; bits++) {
        const uint32_t flags = (bits & 1 ? SERIAL : 0) | (bits & 2 ? LANE : 0) | (bits & 4 ? PKC : 0) | (bits & 8 ? CULL : 0) | (bits & 16 ? CW : 0) |
                               (bits & 32 ? SIMPLE : 0) | (bits & 64 ? PSTAT : 0) | (bits & 128 ? AOV : 0);
        for (int lights : { 1, 33 }) for (int instances : { 1, 2, 65 }) for (int fuse = 0; fuse <= 1; fuse++) for (int split : { 0, 64 })
        for (int merge = 0; merge <= 1; merge++) for (int lane_from : { -1, 0, 5, 11 }) for (int lane_from_any : { -1, 5 }) {
            PlanInputs in = frame(flags);
            in.bounces = L - 1; in.can_spawn = true; in.light_count = lights; in.instance_count = instances;
            in.knobs.fuse_shade = fuse != 0; in.knobs.split_items = split; in.knobs.merge_any = merge != 0;
            in.knobs.lane_from_level = lane_from; in.knobs.lane_from_level_any = lane_from_any;
            const RenderPlan p = plan_render(in);
            plans++;
            CHECK(p.levels == L);
            CHECK(p.n_any >= 1 && p.n_any <= L);
            const bool plain = (flags & (CW | SIMPLE)) != 0;
            for (int l = 0; l < L; l++) {
                const int c = p.closest[l], s = p.shade[l];
                CHECK(c >= CLOSEST_PLAIN && c <= CLOSEST_PACKET_FUSED_CULL && s >= SHADE_NONE && s <= SHADE_AOV_CULL);
                CHECK((c == CLOSEST_PLAIN || c == CLOSEST_PLAIN_COUNT) == plain);              // 0 is a kernel too: only a plain call may hold it
                CHECK((s == SHADE_NONE) == (c == CLOSEST_PACKET_FUSED || c == CLOSEST_PACKET_FUSED_CULL));      // a level without a k_shade launch shaded its own hits
                CHECK((s == SHADE_AOV || s == SHADE_AOV_COUNT || s == SHADE_AOV_CULL) == ((flags & AOV) != 0 && l == 0));
                const int n = plan_stats_n(p, in.batch_tiles * 1024, l);
                CHECK(n >= 1 && n <= p.stats_stride);
            }
            int covered[RTX_MAX_LEVELS] = { 0 };
            int last_after = -1;
            for (int i = 0; i < p.n_any && i < L; i++) {
                const AnyLaunch & a = p.any[i];
                CHECK(a.lo >= 0 && a.lo <= a.hi && a.hi <= L - 1);
                CHECK(a.after_level >= a.hi && a.after_level <= p.levels - 1);      // after the k_shade that filled its last level, and no later than the last one
                CHECK(a.after_level >= last_after); last_after = a.after_level;      // in queueing order
                CHECK(a.stream == (p.overlap ? 1 : 0));
                CHECK(a.kernel >= ANY_PLAIN && a.kernel <= ANY_PACKET_SPLIT && (a.items == 0 || a.kernel == ANY_PACKET_SPLIT));
                if (a.kernel == ANY_PLAIN || a.kernel == ANY_PLAIN_COUNT) CHECK(a.lo == a.hi);      // the plain kernels take lo only
                for (int l = a.lo; l <= a.hi && l < L; l++) if (l >= 0) covered[l]++;
            }
            for (int l = 0; l < L; l++) CHECK(covered[l] == 1);
            if (p.split) CHECK(p.item_cap >= 64 && p.item_cap <= (1 << 16));
        }
    }
    CHECK(plans == 256l * 2 * 3 * 2 * 2 * 2 * 4 * 2);
    {   // the merged launch of the one-stream shape is ONE launch over 0 .. 11, after level 11; the two-stream shape's second launch covers 1 .. 11
        PlanInputs in = frame(SERIAL); in.bounces = L - 1; in.light_count = 33;
        CHECK(schedule(plan_render(in), { { 11, 0, ANY_PACKET_SPLIT, 0, 11, 1 } }));
        in.flags = 0;
        CHECK(schedule(plan_render(in), { { 0, 1, ANY_PACKET_SPLIT, 0, 0, 1 }, { 11, 1, ANY_PACKET_SPLIT, 1, 11, 1 } }));
        in.instance_count = 2; in.knobs.split_items = 0;                 // per-lane from level 2: three launches
        CHECK(schedule(plan_render(in), { { 0, 1, ANY_PACKET, 0, 0, 0 }, { 11, 1, ANY_PACKET, 1, 1, 0 }, { 11, 1, ANY_LANE, 2, 11, 0 } }));
        in.knobs.lane_from_level = 11;                                   // the last level alone goes per lane
        const RenderPlan p = plan_render(in);
        CHECK(p.closest[10] == CLOSEST_PACKET && p.closest[11] == CLOSEST_LANE);
        CHECK(schedule(p, { { 0, 1, ANY_PACKET, 0, 0, 0 }, { 11, 1, ANY_PACKET, 1, 10, 0 }, { 11, 1, ANY_LANE, 11, 11, 0 } }));
        in.flags = SERIAL; in.knobs.merge_any = false;                    // one launch per level: the array is exactly full
        CHECK(plan_render(in).n_any == L);
    }
}

// RTX_PK_LONE_ENTRY: the plan carries the frame's two facts with the knob applied, copy_class never without lone, and either changes the plan's bytes
static void lone_entry() {
    CASE("lone entry");
    PlanInputs in = frame(); in.knobs.lone_entry = true;
    const RenderPlan none = plan_render(in);
    CHECK(!none.lone && !none.copy_class);
    in.lone = true;
    const RenderPlan lone = plan_render(in);
    CHECK(lone.lone == 1 && !lone.copy_class && memcmp(&lone, &none, sizeof(lone)) != 0);
    in.copy_class = true;
    const RenderPlan copy = plan_render(in);
    CHECK(copy.lone == 1 && copy.copy_class == 1 && memcmp(&copy, &lone, sizeof(copy)) != 0);
    in.lone = false;                                                     // a fact the host never states: still no copy_class without lone
    CHECK(!plan_render(in).lone && !plan_render(in).copy_class);
    in.lone = true; in.knobs.lone_entry = false;
    const RenderPlan off = plan_render(in);
    CHECK(!off.lone && !off.copy_class);
    in.lone = false; in.copy_class = false;
    const RenderPlan off_none = plan_render(in);
    CHECK(memcmp(&off, &off_none, sizeof(off)) == 0);                    // nothing else of the plan depends on the facts
}

int main() {
    lone_entry();
    small_grids();
    twelve_levels();
    modes_and_schedule();
    instrumented_modes();
    stack_limits();
    two_deep_trees();
    lpt_items_graph();
    if (failures) { printf("plan_check: %d FAILED\n", failures); return 1; }
    printf("plan_check: ok\n");
    return 0;
}
