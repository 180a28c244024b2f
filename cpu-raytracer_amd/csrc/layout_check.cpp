// layout_check.cpp — the device node layouts of rtx_layout.h on the CPU: `make layout_check` builds this with -fsanitize=address,undefined
// and runs it.  The traversal kernels read these records with hand-written assembly, so a record writer that drifts is a wrong image only
// some scenes show.  Pinned here, bit for bit: the records of small trees spelled out by hand, the lane record's round trip, the packed stack
// and work-list entries of the per-lane walks (round trip at the field limits, the fit rules, the pk4c slot's reference), and that the
// pass a refit and a build end with (rtxl::finish_index, the body of k_refit_finish / k_build_finish) gives back exactly what the host
// converters of rtx_layout_host.h made — which is what plan_refit relies on when it runs the pass at bind, and where the pk4c meta word
// composed from slot-index arithmetic meets the one composed from the tree walk.  Needs no GPU and no ROCm.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "rtx_layout_host.h"

static int failures = 0;
static const char * current = "";
#define CASE(name) current = name
#define CHECK(x) do { if (!(x)) { printf("FAILED [%s] line %d: %s\n", current, __LINE__, #x); failures++; } } while (0)

static const int MAX_NEED = 36;                    // RTX_PK4_MAX_NEED of rtx_packet.h: bounds a schedule, shapes no record
enum { AXIS_X = 1, AXIS_Y = 2, AXIS_Z = 3 };

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(const std::vector<Quad> & a, const std::vector<Quad> & b) { return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(Quad)) == 0; }

// one row of 8 words as written out by hand: (min.x, min.y, max.x, max.y, min.z, max.z) and two integer words
struct Row { float f[6]; uint32_t w6, w7; };
static const Row ZERO = { { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, 0u, 0u };
static bool row_is(const std::vector<Quad> & rows, size_t i, const Row & want) {
    uint32_t got[8], w[8];
    memcpy(got, &rows[2 * i], 32);
    for (int k = 0; k < 6; k++) w[k] = bits(want.f[k]);
    w[6] = want.w6; w[7] = want.w7;
    return memcmp(got, w, 32) == 0;
}

static rtx_bvh_node node(float x0, float y0, float z0, float x1, float y1, float z1, int32_t left_or_first, uint32_t count) {
    rtx_bvh_node n;
    n.aabb_min[0] = x0; n.aabb_min[1] = y0; n.aabb_min[2] = z0; n.aabb_max[0] = x1; n.aabb_max[1] = y1; n.aabb_max[2] = z1;
    n.left_or_first = left_or_first; memcpy(&n.count, &count, 4);
    return n;
}

// ---- the records of two small balanced shapes, word by word (the rows tests/test_layouts_cpu.py spells in numpy) ---------------------------
static void hand_spelled_records() {
    CASE("5 triangles: packet, pk4 and pk4c records by hand");
    {   // root [0, 5) at 0, leaves [0, 2) and [2, 5) at 2 and 3, index 1 unused; a -0.0, a repeated plane and a denormal among the coordinates
        const rtx_bvh_node zero = node(0, 0, 0, 0, 0, 0, 0, 0u);
        const rtx_bvh_node tree[4] = { node(-2.0f, -1.0f, -0.0f, 3.0f, 1.5f, 4.0f, 2, (uint32_t)AXIS_Y << 30), zero,
                                       node(-2.0f, -1.0f, 0.5f, 0.25f, 1.5f, 4.0f, 0, 2u), node(0.25f, -0.5f, -0.0f, 3.0f, 1.0f, 1e-40f, 2, 3u) };
        const Row r0 = { { -2.0f, -1.0f, 3.0f, 1.5f, -0.0f, 4.0f }, 2u, 0x80000000u };
        const Row r2 = { { -2.0f, -1.0f, 0.25f, 1.5f, 0.5f, 4.0f }, 0u, 2u };
        const Row r3 = { { 0.25f, -0.5f, 3.0f, 1.0f, -0.0f, 1e-40f }, 2u, 3u };
        CHECK(bits(r3.f[5]) == 0x000116c2u && bits(r0.f[4]) == 0x80000000u);      // the denormal and the -0.0 are what they say
        std::vector<Quad> lane, pk, pk4, pk4c;
        int need = -1;
        convert_nodes(tree, 4, lane); convert_nodes_pk(tree, 4, pk);
        CHECK(pk.size() == 8 && row_is(pk, 0, r0) && row_is(pk, 1, ZERO) && row_is(pk, 2, r2) && row_is(pk, 3, r3));
        const uint32_t lane0[8] = { bits(-2.0f), bits(-1.0f), bits(-0.0f), 2u, bits(3.0f), bits(1.5f), bits(4.0f), 0x80000000u };
        CHECK(lane.size() == 8 && memcmp(&lane[0], lane0, 32) == 0);
        CHECK(build_nodes_pk4(tree, 4, 5, pk4, &need, 1, MAX_NEED) && need == 1 && pk4.size() == 24);      // largest box first: node 2, then node 3
        CHECK(build_nodes_pk4c(tree, 4, 5, pk4c, &need) && need == 1 && pk4c.size() == 24);
        for (size_t i = 0; i < 12; i++) {
            CHECK(row_is(pk4, i, i == 4 ? r2 : i == 5 ? r3 : ZERO));
            CHECK(row_is(pk4c, i, i == 4 ? r2 : i == 6 ? r3 : ZERO));   // a leaf child sits alone in the first slot of its pair
        }
    }
    CASE("9 triangles: the root's pk4c record carries a parent axis");
    {   // root at 0; 2 the leaf [0, 4); 3 inner (axis z) over its leaves [4, 6) and [6, 9) at 6 and 7; 1, 4 and 5 are holes
        const rtx_bvh_node zero = node(0, 0, 0, 0, 0, 0, 0, 0u);
        const rtx_bvh_node tree[8] = { node(-4.0f, -3.0f, -2.0f, 4.0f, 3.0f, 2.0f, 2, (uint32_t)AXIS_X << 30), zero, node(-4.0f, -3.0f, -2.0f, -1.0f, 0.0f, 2.0f, 0, 4u),
                                       node(-1.5f, -2.5f, -1.0f, 4.0f, 3.0f, 1.75f, 6, (uint32_t)AXIS_Z << 30), zero, zero,
                                       node(-1.5f, -2.5f, -1.0f, 1.0f, 3.0f, 0.0f, 4, 2u), node(0.5f, -2.0f, -0.5f, 4.0f, 2.0f, 1.75f, 6, 3u) };
        const Row r2 = { { -4.0f, -3.0f, -1.0f, 0.0f, -2.0f, 2.0f }, 0u, 4u };
        const Row r6 = { { -1.5f, -2.5f, 1.0f, 3.0f, -1.0f, 0.0f }, 4u, 2u }, r6_under_root = { { -1.5f, -2.5f, 1.0f, 3.0f, -1.0f, 0.0f }, 4u, 2u | 3u << 26 };
        const Row r7 = { { 0.5f, -2.0f, 4.0f, 2.0f, -0.5f, 1.75f }, 6u, 3u };
        std::vector<Quad> pk4c;
        int need = -1;
        CHECK(build_nodes_pk4c(tree, 8, 9, pk4c, &need) && need == 2 && pk4c.size() == 40);
        CHECK(row_is(pk4c, 4, r2) && row_is(pk4c, 5, ZERO) && row_is(pk4c, 6, r6_under_root) && row_is(pk4c, 7, r7));
        CHECK(row_is(pk4c, 12, r6) && row_is(pk4c, 13, ZERO) && row_is(pk4c, 14, r7) && row_is(pk4c, 15, ZERO));      // node 3's own record: two leaf children, no parent axis
    }
    CASE("pk4c meta word");
    CHECK(rtxl::pk4c_meta(3u, 3u, 0) == 3u && rtxl::pk4c_meta(3u, 3u, 2) == 3u);                                    // the slot is a leaf child of the record's node
    CHECK(rtxl::pk4c_meta(2u, 3u << 30, 0) == (2u | 3u << 26) && rtxl::pk4c_meta(2u, 3u << 30, 1) == 2u);          // the parent's axis rides in the first slot of the pair
    CHECK(rtxl::pk4c_meta(1u << 30, 2u << 30, 2) == (2u << 26 | 1u << 30) && rtxl::pk4c_meta(1u << 30, 2u << 30, 3) == 1u << 30);
    CHECK(rtxl::pk4c_meta(5u | 2u << 30, 5u | 2u << 30, 0) == (5u | 2u << 30));                                     // a leaf's own axis bits are its own, never a parent's
}

// ---- the packed stack and work-list entries of the per-lane walks ----------------------------------------------------------------------------
static void packed_entries() {
    CASE("leaf reference: round trip at the field limits, the fit rule, the bits the asm walkers spell");
    const uint32_t first_max = (1u << 24) - 1u;
    for (uint32_t axis = 0; axis <= 3u; axis++)
        for (uint32_t leaf : { 0u, 1u, 15u })
            for (uint32_t first : { 0u, 1u, first_max }) {
                const uint32_t cw = leaf | axis << 30;
                CHECK(rtxl::ref_fits(first, cw));
                const int32_t e = rtxl::ref_pack(first, cw);
                CHECK((uint32_t)e == (0x40000000u | axis << 28 | leaf << 24 | first));
                CHECK(rtxl::ref_is_packed(e) && e > 0 && (uint32_t)rtxl::ref_first(e) == first && (uint32_t)rtxl::ref_count_word(e) == cw);
            }
    CHECK((uint32_t)rtxl::ref_pack(first_max, 15u | 3u << 30) == 0x7fffffffu && rtxl::REF_PACKED == 0x40000000u);
    CHECK(!rtxl::ref_fits(1u << 24, 1u) && !rtxl::ref_fits(0u, 16u) && !rtxl::ref_fits(0u, 16u | 3u << 30) && !rtxl::ref_fits(0xffffffffu, 0u));
    CHECK(!rtxl::ref_is_packed((int32_t)first_max) && !rtxl::ref_is_packed(0));          // a node index is never taken for a packed reference
    CASE("leaf reference of a pk4c slot equals the one of its node's (first, count)");
    for (int s = 0; s < 4; s++)
        for (uint32_t child_count : { 3u, 1u << 30, 3u << 30 })
            for (uint32_t slot_count : { 15u, 1u, 2u << 30, 3u << 30 }) {
                const uint32_t meta = rtxl::pk4c_meta(slot_count, child_count, s);
                CHECK(rtxl::ref_pack_meta(first_max, meta) == rtxl::ref_pack(first_max, slot_count));
                CHECK(rtxl::ref_pack_meta(6u, meta) == rtxl::ref_pack(6u, slot_count));
            }
    CHECK(rtxl::pk4c_meta(2u, 3u << 30, 0) != 2u && rtxl::ref_pack_meta(4u, rtxl::pk4c_meta(2u, 3u << 30, 0)) == (int32_t)(0x40000000u | 2u << 24 | 4u));   // a parent axis rode in that meta word
    CASE("4-wide entry: round trip at the field limits, the fit rule");
    for (uint32_t count : { 0u, 1u, 255u })
        for (uint32_t first : { 0u, 1u, first_max }) {
            CHECK(rtxl::wide_fits(first, count));
            const int32_t e = rtxl::wide_pack(first, count);
            CHECK((uint32_t)e == (count << 24 | first) && (uint32_t)rtxl::wide_first(e) == first && (uint32_t)rtxl::wide_count(e) == count);
        }
    CHECK((uint32_t)rtxl::wide_pack(first_max, 255u) == 0xffffffffu);
    CHECK(!rtxl::wide_fits(1u << 24, 1u) && !rtxl::wide_fits(0u, 256u));
}

// ---- the lane record's inverse --------------------------------------------------------------------------------------------------------------
static void lane_round_trip() {
    CASE("lane record round trip");
    const float nan_a = from_bits(0x7fc12345u), nan_b = from_bits(0xffc00001u), nan_c = from_bits(0x7fffffffu);
    const rtx_bvh_node in[4] = { node(nan_a, -0.0f, 1e-40f, nan_b, from_bits(0x7f800000u), nan_c, 0x00fffffe, 3u << 30),
                                 node(1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f, -1, 0xffffffffu),
                                 node(-1.0f, nan_c, from_bits(0xff800000u), nan_a, -2.0f, nan_b, 7, 15u | 2u << 30),      // a leaf's count word with axis bits set
                                 node(0, 0, 0, 0, 0, 0, 0, 0u) };
    std::vector<Quad> lane;
    convert_nodes(in, 4, lane);
    rtx_bvh_node out[4];
    memset(out, 0xab, sizeof(out));
    for (int i = 0; i < 4; i++) rtxl::node_from_lane(lane.data(), i, out[i]);
    CHECK(memcmp(in, out, sizeof(in)) == 0);
    CHECK(bits(lane[0].x) == 0x7fc12345u && bits(lane[0].w) == 0x00fffffeu && bits(lane[1].x) == 0xffc00001u && bits(lane[1].w) == 0xc0000000u);
    const rtxu::Box b = rtxl::load_box(lane.data(), 2);
    CHECK(bits(b.mn[1]) == 0x7fffffffu && bits(b.mn[2]) == 0xff800000u && bits(b.mx[0]) == 0x7fc12345u && bits(b.mx[2]) == 0xffc00001u);
}

// ---- finish is the identity on converted arrays ---------------------------------------------------------------------------------------------
struct HostView {                                   // DevRefit's like on the host
    Quad * nodes, * pk_nodes, * pk4_nodes, * pk4c_nodes;
    const int32_t * parent, * map4, * map4c;
    float * plane_keys[3];
    int32_t node_count;
};

static void finish_is_identity(const char * name, const std::vector<rtx_bvh_node> & tree, int tri_count, int order_mode) {
    CASE(name);
    const int n = (int)tree.size();
    std::vector<Quad> lane, pk, pk4, pk4c;
    std::vector<int32_t> map4, map4c, parent;
    int need4 = -1, need4c = -1;
    convert_nodes(tree.data(), n, lane); convert_nodes_pk(tree.data(), n, pk);
    CHECK(build_nodes_pk4(tree.data(), n, tri_count, pk4, &need4, order_mode, MAX_NEED, &map4));
    CHECK(build_nodes_pk4c(tree.data(), n, tri_count, pk4c, &need4c, &map4c));
    if (failures) return;
    parent_table(lane.data(), n, parent);
    for (int i = 0; i < n; i++) { rtx_bvh_node back; rtxl::node_from_lane(lane.data(), i, back); CHECK(memcmp(&back, &tree[i], sizeof(back)) == 0); }
    std::vector<float> keys[3];                     // restated: every slot's (min, max) per axis, a NaN as +inf
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < n; i++) for (int e = 0; e < 2; e++) { const float v = e ? tree[i].aabb_max[a] : tree[i].aabb_min[a]; keys[a].push_back((bits(v) & 0x7fffffffu) > 0x7f800000u ? from_bits(0x7f800000u) : v); }
    const float junk = from_bits(0xdeadbeefu), stays = from_bits(0x5a5a5a5au);
    for (int axis_fields = 0; axis_fields <= 1; axis_fields++) {
        // everything the pass must write starts as junk: the packet records of reachable nodes, the boxes of used wide slots (their first
        // words stay, and the meta words unless the pass is to compose them), every plane key; what it must leave alone is marked
        std::vector<Quad> g_lane = lane, g_pk = pk, g_pk4 = pk4, g_pk4c = pk4c;
        std::vector<float> g_keys[3];
        int reachable = 0, used4 = 0, used4c = 0;
        std::vector<Quad> want_pk = pk;             // an unreachable slot keeps its bytes, whatever they are
        for (int i = 0; i < n; i++) {
            if (parent[i] != RTX_REFIT_UNREACHABLE) { g_pk[2 * i] = g_pk[2 * i + 1] = Quad{ junk, junk, junk, junk }; reachable++; }
            else g_pk[2 * i] = g_pk[2 * i + 1] = want_pk[2 * i] = want_pk[2 * i + 1] = Quad{ stays, stays, stays, stays };
        }
        for (int s = 0; s < 2 * n + 4; s++) {
            if (map4[s] >= 0) { g_pk4[2 * s] = Quad{ junk, junk, junk, junk }; g_pk4[2 * s + 1].x = g_pk4[2 * s + 1].y = junk; used4++; }
            if (map4c[s] >= 0) { g_pk4c[2 * s] = Quad{ junk, junk, junk, junk }; g_pk4c[2 * s + 1].x = g_pk4c[2 * s + 1].y = junk; if (axis_fields) g_pk4c[2 * s + 1].w = junk; used4c++; }
        }
        for (int a = 0; a < 3; a++) g_keys[a].assign((size_t)2 * n, junk);
        CHECK(reachable >= 1 && used4 == used4c && (used4 > 0) == (reachable > 1));
        HostView v = { g_lane.data(), g_pk.data(), g_pk4.data(), g_pk4c.data(), parent.data(), map4.data(), map4c.data(), { g_keys[0].data(), g_keys[1].data(), g_keys[2].data() }, n };
        for (int i = 0; i < 2 * n + 4; i++) rtxl::finish_index(v, i, axis_fields != 0);
        CHECK(same(g_lane, lane));
        CHECK(same(g_pk, want_pk));
        CHECK(same(g_pk4, pk4));
        CHECK(same(g_pk4c, pk4c));
        for (int a = 0; a < 3; a++) CHECK(memcmp(g_keys[a].data(), keys[a].data(), (size_t)2 * n * 4) == 0);
    }
}

// the balanced topology of T triangles with the boxes the host twin (rtxh_blas_build_balanced) would give it: slot k holds triangle k of a
// deterministic soup; leaves from their slots, inner nodes from their children's stored boxes, deepest level first
static std::vector<rtx_bvh_node> balanced_tree(int T) {
    std::vector<float> v((size_t)9 * T);
    uint32_t seed = 12345u + (uint32_t)T;
    for (float & x : v) { seed = seed * 1664525u + 1013904223u; x = (float)(int32_t)(seed >> 8 & 0xffffu) / 4096.0f - 8.0f; }
    std::vector<rtx_bvh_node> nodes;
    balanced_topology(T, nodes);
    auto load = [&](int i) { rtxu::Box b; memcpy(b.mn, nodes[i].aabb_min, 12); memcpy(b.mx, nodes[i].aabb_max, 12); return b; };
    for (int d = rtxb::tree_levels(T); d >= 0; d--)
        for (int j = 0; j < (1 << d); j++) {
            int first;
            const int cnt = rtxb::node_range(T, d, j, &first), slot = rtxu::node_slot(d, j);
            if (cnt == 0) continue;
            rtxu::Box b;
            if (cnt <= RTX_BUILD_LEAF_MAX) {
                b = rtxr::empty_box();
                for (int k = first; k < first + cnt; k++) rtxr::expand_box(b, rtxr::triangle_box(&v[9 * (size_t)k], &v[9 * (size_t)k + 3], &v[9 * (size_t)k + 6]));
                rtxr::finish_leaf(b);
            } else {
                const rtxu::Box l = load(nodes[slot].left_or_first), r = load(nodes[slot].left_or_first + 1);
                b = rtxr::join_children(l, r);
                nodes[slot].count = (int32_t)((uint32_t)rtxb::join_axis(l, r) << 30);
            }
            memcpy(nodes[slot].aabb_min, b.mn, 12); memcpy(nodes[slot].aabb_max, b.mx, 12);
        }
    return nodes;
}

// an unbalanced tree in the reference's array shape: index 1 unused (garbage with a NaN), a leaf directly under the root beside a chain
static std::vector<rtx_bvh_node> unbalanced_tree() {
    const float q = from_bits(0x7fc00abcu);
    return { node(-4.0f, -4.0f, -4.0f, 4.0f, 4.0f, 4.0f, 2, (uint32_t)AXIS_X << 30),
             node(q, 9.0f, -9.0f, 9.0f, q, 7.0f, 0x12345678, 0x9abcdef0u),
             node(-4.0f, -4.0f, -3.0f, -1.0f, 4.0f, 4.0f, 0, 3u),                                  // 2: a leaf, the root's left child
             node(-1.0f, -3.5f, -4.0f, 4.0f, 3.0f, 3.5f, 4, (uint32_t)AXIS_Z << 30),              // 3: inner
             node(-1.0f, -3.5f, -4.0f, 2.0f, 3.0f, 0.5f, 6, (uint32_t)AXIS_Y << 30),              // 4: inner
             node(1.0f, -2.0f, -0.0f, 4.0f, 2.5f, 3.5f, 3, 2u),                                    // 5: leaf
             node(-1.0f, -3.5f, -4.0f, 0.5f, 0.0f, 0.5f, 5, 1u),                                   // 6: leaf
             node(0.0f, -1.0f, -2.0f, 2.0f, 3.0f, 0.0f, 6, 4u) };                                  // 7: leaf
}

int main() {
    hand_spelled_records();
    lane_round_trip();
    packed_entries();
    for (int T : { 1, 4, 5, 9, 16, 17, 1025 })
        for (int order_mode = 0; order_mode <= 1; order_mode++) {
            char name[64];
            snprintf(name, sizeof(name), "finish on the balanced tree of %d triangles, pk4 order %d", T, order_mode);
            finish_is_identity(name, balanced_tree(T), T, order_mode);
        }
    {
        const std::vector<rtx_bvh_node> tree = unbalanced_tree();
        finish_is_identity("finish on an unbalanced tree, a leaf under the root", tree, 10, 1);
        CASE("the unbalanced tree's meta words by hand");
        std::vector<Quad> pk4c; int need = -1;
        CHECK(build_nodes_pk4c(tree.data(), 8, 10, pk4c, &need));
        CHECK(bits(pk4c[2 * 4 + 1].w) == 3u && bits(pk4c[2 * 5 + 1].w) == 0u);                                              // the root's record: the leaf child alone
        CHECK(bits(pk4c[2 * 6 + 1].w) == (3u << 26 | 2u << 30) && bits(pk4c[2 * 7 + 1].w) == 2u);                           // node 4 under node 3 (z), its own axis y; leaf 5
        CHECK(bits(pk4c[2 * 8 + 1].w) == (1u | 2u << 26) && bits(pk4c[2 * 9 + 1].w) == 4u && bits(pk4c[2 * 10 + 1].w) == 2u); // node 3's record: 6 and 7 under node 4 (y), leaf 5
    }
    if (failures) { printf("layout_check: %d FAILED\n", failures); return 1; }
    printf("layout_check: ok\n");
    return 0;
}
