// hits_check.cpp — the walk of rtx_query_hits (rtx_hits_math.h) against the exhaustive search over the same hit tests, on generated trees,
// under the host sanitizers (make hits_check).  No GPU, no ROCm.
//   trees      chains (every inner node = one leaf + the rest), combs (the leaf alternates sides) and balanced trees, for the BLAS and the
//              TLAS, up to the stack bound of RTX_MAX_STACK entries; leaves of 1 .. 4 slots
//   triangles  slabs stacked along x (a ray along x crosses dozens: rows with far more than K hits), random ones, duplicated slots, degenerate
//              and NaN triangles
//   instances  translated, rotated, and coincident pairs (same mesh, same matrix: equal t, the order rule decides); spheres and planes
//   checked    K in {1, 8}, with and without a count: every listed hit is in the exhaustive list with the same bits; the list ascends under
//              the order rule; count <= the exhaustive count; the list of K = 1 is the head of the list of K = 8 when both count (one node
//              set); the stack never above rtxnp::stack_need; dead rows have count 0 and an empty list; spheres and planes exactly
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_hits_math.h"

using rtxnp::P3;

static uint32_t rng_state = 24680u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.0f / 16777216.0f); }
static float rnd(float lo, float hi) { return lo + (hi - lo) * rnd(); }
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Mesh { std::vector<rtx_bvh_node> nodes; std::vector<rtx_triangle_hot> hot; int inner_depth = -1; };
struct Scene {
    std::vector<Mesh> meshes; std::vector<rtx_instance> inst; std::vector<rtx_bvh_node> tlas; std::vector<int32_t> tlas_idx;
    std::vector<rtx_sphere> spheres; std::vector<rtx_plane> planes; int tlas_depth = -1;
};
struct Box { float mn[3], mx[3]; };
static Box empty_box() { Box b; for (int a = 0; a < 3; a++) { b.mn[a] = INFINITY; b.mx[a] = -INFINITY; } return b; }
static void grow(Box & b, const float p[3]) { for (int a = 0; a < 3; a++) { if (p[a] < b.mn[a]) b.mn[a] = p[a]; if (p[a] > b.mx[a]) b.mx[a] = p[a]; } }
static void merge(Box & b, const Box & o) { grow(b, o.mn); grow(b, o.mx); }
static Box tri_box(const rtx_triangle_hot & t) {
    Box b = empty_box();
    float q[3];
    grow(b, t.position_0);
    for (int a = 0; a < 3; a++) q[a] = t.position_0[a] + t.position_edge_1[a];
    grow(b, q);
    for (int a = 0; a < 3; a++) q[a] = t.position_0[a] + t.position_edge_2[a];
    grow(b, q);
    return b;                                   // a NaN vertex leaves the box without it: NaN compares false
}

enum { CHAIN = 0, COMB = 1, BALANCED = 2 };
static Box build(std::vector<rtx_bvh_node> & nodes, int self, const std::vector<Box> & prims, int lo, int hi, int shape, int leaf_max, int depth, int & inner_depth) {
    Box b = empty_box();
    if (hi - lo <= leaf_max) {
        for (int i = lo; i < hi; i++) merge(b, prims[i]);
        nodes[self].left_or_first = lo; nodes[self].count = hi - lo;
    } else {
        if (depth > inner_depth) inner_depth = depth;
        const int left = (int)nodes.size();
        nodes.push_back(rtx_bvh_node()); nodes.push_back(rtx_bvh_node());
        const int mid = shape == BALANCED ? (lo + hi) / 2 : (shape == CHAIN || (depth & 1)) ? lo + leaf_max : hi - leaf_max;
        const Box l = build(nodes, left, prims, lo, mid, shape, leaf_max, depth + 1, inner_depth);
        const Box r = build(nodes, left + 1, prims, mid, hi, shape, leaf_max, depth + 1, inner_depth);
        merge(b, l); merge(b, r);
        nodes[self].left_or_first = left; nodes[self].count = (int32_t)((uint32_t)(1 + depth % 3) << 30);
    }
    memcpy(nodes[self].aabb_min, b.mn, 12); memcpy(nodes[self].aabb_max, b.mx, 12);
    return b;
}

// slab i of n: a large triangle across the x axis at x ~ -4 + 8 i / n, tilted a little, so that rays along x cross most of them
static rtx_triangle_hot slab_triangle(int i, int n) {
    rtx_triangle_hot t;
    const float x = -4.0f + 8.0f * (float)i / (float)n;
    t.position_0[0] = x + rnd(-0.01f, 0.01f); t.position_0[1] = rnd(-3.0f, -2.0f); t.position_0[2] = rnd(-3.0f, -2.0f);
    t.position_edge_1[0] = rnd(-0.05f, 0.05f); t.position_edge_1[1] = rnd(5.0f, 7.0f); t.position_edge_1[2] = rnd(-0.5f, 0.5f);
    t.position_edge_2[0] = rnd(-0.05f, 0.05f); t.position_edge_2[1] = rnd(-0.5f, 0.5f); t.position_edge_2[2] = rnd(5.0f, 7.0f);
    return t;
}
static Mesh make_mesh(int n, int shape, int leaf_max, bool hostile, bool slabs) {
    Mesh m;
    for (int i = 0; i < n; i++) {
        rtx_triangle_hot t;
        if (slabs) t = slab_triangle(i, n);
        else for (int a = 0; a < 3; a++) { t.position_0[a] = rnd(-4.0f, 4.0f); t.position_edge_1[a] = rnd(-2.0f, 2.0f); t.position_edge_2[a] = rnd(-2.0f, 2.0f); }
        if (hostile) {
            const int k = i % 7;
            if (k == 1 && i > 0) t = m.hot[i - 1];                                                     // a duplicated slot: two hits at one t
            if (k == 2) for (int a = 0; a < 3; a++) t.position_edge_1[a] = 0.0f;                       // a zero edge: a = 0, f = inf, NaN
            if (k == 3) for (int a = 0; a < 3; a++) t.position_edge_2[a] = 2.0f * t.position_edge_1[a]; // parallel edges
            if (k == 5) t.position_0[i % 3] = NAN;                                                      // a pad triangle of rtx_build_blas
        }
        m.hot.push_back(t);
    }
    std::vector<Box> prims;
    for (const rtx_triangle_hot & t : m.hot) prims.push_back(tri_box(t));
    m.nodes.push_back(rtx_bvh_node());
    build(m.nodes, 0, prims, 0, n, shape, leaf_max, 0, m.inner_depth);
    return m;
}
static void identity(float m[16]) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
static rtx_instance make_instance(int blas, float angle, const float t[3]) {      // rotation about z, then translation: world and its inverse
    rtx_instance I; memset(&I, 0, sizeof(I));
    I.blas_id = blas;
    identity(I.world); identity(I.world_inv);
    const float c = cosf(angle), s = sinf(angle);
    if (angle != 0.0f) {
        I.world[0] = c; I.world[1] = -s; I.world[4] = s; I.world[5] = c;
        I.world_inv[0] = c; I.world_inv[1] = s; I.world_inv[4] = -s; I.world_inv[5] = c;
    }
    I.world[3] = t[0]; I.world[7] = t[1]; I.world[11] = t[2];
    I.world_inv[3] = -(I.world_inv[0] * t[0] + I.world_inv[1] * t[1]); I.world_inv[7] = -(I.world_inv[4] * t[0] + I.world_inv[5] * t[1]); I.world_inv[11] = -t[2];
    return I;
}
static Box instance_box(const Scene & s, const rtx_instance & I) {
    const rtx_bvh_node & r = s.meshes[I.blas_id].nodes[0];
    Box b = empty_box();
    for (int k = 0; k < 8; k++) {
        const P3 c = rtxnp::mk((k & 1) ? r.aabb_max[0] : r.aabb_min[0], (k & 2) ? r.aabb_max[1] : r.aabb_min[1], (k & 4) ? r.aabb_max[2] : r.aabb_min[2]);
        const P3 w = rtxnp::xform_pos(I.world, c);
        const float q[3] = { w.x, w.y, w.z };
        grow(b, q);
    }
    return b;
}
static void make_tlas(Scene & s, int shape, int leaf_max) {
    std::vector<Box> prims;
    for (size_t i = 0; i < s.inst.size(); i++) { prims.push_back(instance_box(s, s.inst[i])); s.tlas_idx.push_back((int32_t)i); }
    s.tlas.push_back(rtx_bvh_node());
    build(s.tlas, 0, prims, 0, (int)prims.size(), shape, leaf_max, 0, s.tlas_depth);
}

struct Access {
    const Scene & s; const Mesh * M = nullptr;
    RTX_WALK_UNFILTERED
    int instance_count() const { return (int)s.inst.size(); }
    int sphere_count() const { return (int)s.spheres.size(); }
    int plane_count() const { return (int)s.planes.size(); }
    int tlas_nodes() const { return (int)s.tlas.size(); }
    void sphere(int i, P3 & c, float & r2) const { c = rtxnp::ptr3(s.spheres[i].center); r2 = s.spheres[i].radius_squared; }
    void plane(int i, P3 & n, float & d) const { n = rtxnp::ptr3(s.planes[i].normal); d = s.planes[i].distance; }
    static void node(const rtx_bvh_node & nd, P3 & mn, P3 & mx, int & first, int & count) { mn = rtxnp::ptr3(nd.aabb_min); mx = rtxnp::ptr3(nd.aabb_max); first = nd.left_or_first; count = nd.count; }
    void tlas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(s.tlas.at(i), mn, mx, f, c); }
    void blas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(M->nodes.at(i), mn, mx, f, c); }
    int enter(int slot, P3 o, P3 d, P3 & co, P3 & cd) {
        const int inst = s.tlas_idx.at(slot);
        co = rtxnp::xform_pos(s.inst[inst].world_inv, o); cd = rtxnp::xform_dir(s.inst[inst].world_inv, d);
        M = &s.meshes[s.inst[inst].blas_id];
        return inst;
    }
    void triangle(int i, P3 & p0, P3 & e1, P3 & e2) const { const rtx_triangle_hot & t = M->hot.at(i); p0 = rtxnp::ptr3(t.position_0); e1 = rtxnp::ptr3(t.position_edge_1); e2 = rtxnp::ptr3(t.position_edge_2); }
};
struct Stack {
    std::vector<int> node; std::vector<float> key; int high = 0;
    explicit Stack(int cap) : node(cap), key(cap) {}
    void push(int sp, int n, float k) { node.at(sp) = n; key.at(sp) = k; if (sp + 1 > high) high = sp + 1; }      // at(): beyond the stated count is a failure
    void pop(int sp, int & n, float & k) const { n = node.at(sp); k = key.at(sp); }
};
struct Hit { float t; int32_t object, triangle; };
struct List {                                   // K entries: at() beyond them is a failure
    std::vector<Hit> h;
    explicit List(int K) : h(K > 0 ? K : 0) {}
    void get(int j, float & t, int32_t & o, int32_t & s) const { const Hit & x = h.at(j); t = x.t; o = x.object; s = x.triangle; }
    void set(int j, float t, int32_t o, int32_t s) { Hit & x = h.at(j); x.t = t; x.object = o; x.triangle = s; }
};
static bool same_bits(float a, float b) { return rtxnp::float_bits(a) == rtxnp::float_bits(b); }

static std::vector<Hit> exhaustive(const Scene & s, const float * row) {
    std::vector<Hit> all;
    if (!rtxhp::row_is_live(row)) return all;
    const P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
    const float D = row[6];
    const int ic = (int)s.inst.size(), sn = (int)s.spheres.size();
    for (int k = 0; k < sn; k++) {
        float t0, t1;
        if (!rtxhp::sphere_roots(rtxnp::ptr3(s.spheres[k].center), s.spheres[k].radius_squared, o, d, t0, t1)) continue;
        if (rtxhp::in_range(t0, D)) all.push_back(Hit{ t0, ic + k, -1 });
        if (rtxhp::in_range(t1, D)) all.push_back(Hit{ t1, ic + k, -1 });
    }
    for (size_t k = 0; k < s.planes.size(); k++) {
        const float t = rtxhp::plane_t(rtxnp::ptr3(s.planes[k].normal), s.planes[k].distance, o, d);
        if (rtxhp::in_range(t, D)) all.push_back(Hit{ t, ic + sn + (int)k, -1 });
    }
    for (int k = 0; k < ic; k++) {
        const P3 co = rtxnp::xform_pos(s.inst[k].world_inv, o), cd = rtxnp::xform_dir(s.inst[k].world_inv, d);
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t i = 0; i < M.hot.size(); i++) {
            float t, u, v;
            if (rtxhp::tri_test(rtxnp::ptr3(M.hot[i].position_0), rtxnp::ptr3(M.hot[i].position_edge_1), rtxnp::ptr3(M.hot[i].position_edge_2), co, cd, D, t, u, v))
                all.push_back(Hit{ t, k, (int32_t)i });
        }
    }
    std::stable_sort(all.begin(), all.end(), [](const Hit & a, const Hit & b) { return rtxhp::before(a.t, a.object, a.triangle, b.t, b.object, b.triangle); });
    return all;
}

static int worst_stack = 0, most_hits = 0;
static long rows_checked = 0, rows_over_k = 0, lists_equal = 0, lists_total = 0, hits_missed = 0;

static void check_row(const Scene & s, const char * what, int i, const float * row, int need) {
    const std::vector<Hit> all = exhaustive(s, row);
    rows_checked++;
    if ((int)all.size() > most_hits) most_hits = (int)all.size();
    if (all.size() > 8) rows_over_k++;
    Hit head_counted[2] = { { 0, 0, 0 }, { 0, 0, 0 } }; int held_counted[2] = { 0, 0 }, count_counted[2] = { 0, 0 };
    for (int ki = 0; ki < 2; ki++) for (int counted = 0; counted < 2; counted++) {
        const int K = ki ? 8 : 1;
        Access A{ s }; Stack st(need > 0 ? need : 1); List L(K);
        rtxhp::Tally w;
        rtxhp::walk(A, st, L, row, K, counted != 0, w);
        if (st.high > worst_stack) worst_stack = st.high;
        CHECK(st.high <= need, "%s row %d: stack %d above the stated %d", what, i, st.high, need);
        CHECK(w.held >= 0 && w.held <= K && w.held <= w.count, "%s row %d: held %d of K %d, count %d", what, i, w.held, K, w.count);
        CHECK(w.count <= (int)all.size(), "%s row %d K %d counted %d: count %d above the exhaustive %d", what, i, K, counted, w.count, (int)all.size());
        if (counted) { CHECK(w.held == (w.count < K ? w.count : K), "%s row %d: held %d with count %d, K %d", what, i, w.held, w.count, K); hits_missed += (long)all.size() - w.count; }
        size_t at = 0;                                                            // the list is a subsequence of the sorted exhaustive list, bit for bit
        bool prefix = true;
        for (int j = 0; j < w.held; j++) {
            const Hit & x = L.h[j];
            if (j) CHECK(!rtxhp::before(x.t, x.object, x.triangle, L.h[j - 1].t, L.h[j - 1].object, L.h[j - 1].triangle), "%s row %d K %d: entries %d and %d out of order", what, i, K, j - 1, j);
            while (at < all.size() && !(same_bits(all[at].t, x.t) && all[at].object == x.object && all[at].triangle == x.triangle)) { at++; prefix = false; }
            CHECK(at < all.size(), "%s row %d K %d counted %d: entry %d (t %.9g object %d triangle %d) is no hit of the exhaustive search, or twice in the list", what, i, K, counted, j, x.t, x.object, x.triangle);
            if (at < all.size()) at++;
        }
        if (w.held < K && (size_t)w.held < all.size()) prefix = false;
        lists_total++; lists_equal += prefix;
        if (counted) { held_counted[ki] = w.held; count_counted[ki] = w.count; if (w.held) head_counted[ki] = L.h[0]; }
        // spheres and planes are never behind a box: the first K of them are listed, whatever the triangles do
        if (counted && s.inst.empty()) CHECK(prefix && w.count == (int)all.size(), "%s row %d: spheres and planes exactly", what, i);
    }
    CHECK(count_counted[0] == count_counted[1], "%s row %d: the count depends on K (%d, %d)", what, i, count_counted[0], count_counted[1]);
    CHECK((held_counted[0] > 0) == (held_counted[1] > 0), "%s row %d: K = 1 and K = 8 disagree on a hit", what, i);
    if (held_counted[0] && held_counted[1])
        CHECK(same_bits(head_counted[0].t, head_counted[1].t) && head_counted[0].object == head_counted[1].object && head_counted[0].triangle == head_counted[1].triangle,
              "%s row %d: the list of K = 1 is not the head of the list of K = 8", what, i);
}

static void check_scene(const Scene & s, const char * what, int rows, float reach, bool along_x) {
    int deepest = -1;
    for (const Mesh & m : s.meshes) if (m.inner_depth > deepest) deepest = m.inner_depth;
    const int need = rtxnp::stack_need(s.tlas_depth, deepest);
    CHECK(need <= RTX_MAX_STACK, "%s: the generator exceeded the stack bound (%d)", what, need);
    for (int i = 0; i < rows; i++) {
        float row[7] = { rnd(-reach, reach), rnd(-reach, reach), rnd(-reach, reach), rnd(-1, 1), rnd(-1, 1), rnd(-1, 1), INFINITY };
        if (along_x && i % 3 != 2) { row[0] = -reach; row[1] = rnd(-1, 1); row[2] = rnd(-1, 1); row[3] = rnd(0.5f, 2.0f); row[4] = rnd(-0.05f, 0.05f); row[5] = rnd(-0.05f, 0.05f); }
        if (i % 5 == 1) row[6] = rnd(0.01f, 3.0f * reach);
        if (i % 13 == 4) row[3 + i % 3] = 0.0f;                                    // an axis-aligned component: an infinite inverse
        if (i % 17 == 5 && !s.meshes.empty() && s.meshes[0].hot[0].position_0[0] == s.meshes[0].hot[0].position_0[0]) memcpy(row, s.meshes[0].hot[i % s.meshes[0].hot.size()].position_0, 12);   // starts on a vertex
        check_row(s, what, i, row, need);
        if (i % 7 == 3) {                                                        // the same row with D exactly on its first hit, and one ulp beyond
            const std::vector<Hit> all = exhaustive(s, row);
            if (!all.empty()) {
                row[6] = all[all.size() / 2].t; check_row(s, what, i, row, need);
                row[6] = nextafterf(row[6], INFINITY); check_row(s, what, i, row, need);
            }
        }
    }
}

static void dead_rows(const Scene & s) {
    const float bad[][7] = { { NAN, 0, 0, 1, 0, 0, 1 }, { 0, INFINITY, 0, 1, 0, 0, 1 }, { 0, 0, 0, 0, 0, 0, 1 }, { 0, 0, 0, -0.0f, 0, -0.0f, INFINITY }, { 0, 0, 0, 1, NAN, 0, 1 },
                             { 0, 0, 0, 1, 0, -INFINITY, 1 }, { 0, 0, 0, 1, 0, 0, NAN }, { 0, 0, 0, 1, 0, 0, 0 }, { 0, 0, 0, 1, 0, 0, -0.0f }, { 0, 0, 0, 1, 0, 0, -1 }, { 0, 0, 0, 1, 0, 0, -INFINITY } };
    for (const float * row : bad) {
        CHECK(!rtxhp::row_is_live(row), "row (%g %g %g %g %g %g %g) is dead", row[0], row[1], row[2], row[3], row[4], row[5], row[6]);
        Access A{ s }; Stack st(RTX_MAX_STACK); List L(8);
        rtxhp::Tally w;
        rtxhp::walk(A, st, L, row, 8, true, w);
        CHECK(w.count == 0 && w.held == 0 && st.high == 0, "a dead row was walked");
        rows_checked++;
    }
}

int main() {
    const float zero[3] = { 0, 0, 0 };
    // one instance, every tree shape and leaf size; chains and combs up to the stack bound: 63 leaves of one slot = inner depth 61, need 62
    for (int shape = CHAIN; shape <= BALANCED; shape++)
        for (int leaf = 1; leaf <= 4; leaf++)
            for (int hostile = 0; hostile < 2; hostile++) {
                Scene s;
                const int n = shape == BALANCED ? 200 : 63 * leaf - (leaf > 1 ? 1 : 0);
                s.meshes.push_back(make_mesh(n, shape, leaf, hostile != 0, leaf % 2 == 1));
                s.inst.push_back(make_instance(0, 0.0f, zero));
                make_tlas(s, BALANCED, 1);
                char what[64]; snprintf(what, sizeof what, "shape %d leaf %d hostile %d", shape, leaf, hostile);
                check_scene(s, what, 240, 6.0f, leaf % 2 == 1);
            }
    {   // deep TLAS and deep BLAS together, at the bound exactly: a chain of 32 instances (inner depth 30) over a chain mesh of 34 leaves (32): need 31 + 33 = 64
        Scene s;
        s.meshes.push_back(make_mesh(34, CHAIN, 1, false, true));
        s.meshes.push_back(make_mesh(40, COMB, 2, true, false));
        for (int k = 0; k < 32; k++) { const float t[3] = { rnd(-8, 8), rnd(-2, 2), rnd(-2, 2) }; s.inst.push_back(make_instance(k % 3 == 2 ? 1 : 0, k % 2 ? rnd(-0.3f, 0.3f) : 0.0f, t)); }
        make_tlas(s, CHAIN, 1);
        CHECK(rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth) == RTX_MAX_STACK, "the deep scene sits at the bound (%d)", rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth));
        check_scene(s, "deep TLAS over deep BLAS", 400, 14.0f, true);
        dead_rows(s);
    }
    {   // coincident instances, spheres and planes, TLAS leaves of several instances
        Scene s;
        s.meshes.push_back(make_mesh(120, BALANCED, 3, true, true));
        const float t0[3] = { 1.5f, -0.5f, 0.25f }, t1[3] = { -3.0f, 2.0f, 1.0f };
        s.inst.push_back(make_instance(0, 0.7f, t0)); s.inst.push_back(make_instance(0, 0.7f, t0));      // the same mesh twice in one place
        s.inst.push_back(make_instance(0, 0.0f, t1)); s.inst.push_back(make_instance(0, 0.0f, t1));
        s.inst.push_back(make_instance(0, -1.1f, zero));
        make_tlas(s, COMB, 2);
        rtx_sphere sp; memset(&sp, 0, sizeof sp); sp.center[0] = 2; sp.center[1] = 0.5f; sp.center[2] = -0.5f; sp.radius_squared = 2.25f; sp.radius_inv = 1.0f / 1.5f;
        s.spheres.push_back(sp); s.spheres.push_back(sp);
        rtx_plane pl; memset(&pl, 0, sizeof pl); pl.normal[0] = 1.0f; pl.distance = -7.0f; pl.u_axis[1] = 1.0f; pl.v_axis[2] = 1.0f;
        s.planes.push_back(pl);
        check_scene(s, "coincident instances, spheres, planes", 900, 9.0f, true);
        dead_rows(s);
    }
    {   // spheres and planes alone: no TLAS, every hit listed exactly; a ray through a sphere counts twice, from inside once
        Scene s;
        rtx_sphere sp; memset(&sp, 0, sizeof sp); sp.radius_squared = 4.0f; sp.radius_inv = 0.5f;
        s.spheres.push_back(sp);
        rtx_plane pl; memset(&pl, 0, sizeof pl); pl.normal[0] = 1.0f; pl.distance = -5.0f;
        s.planes.push_back(pl);
        check_scene(s, "spheres and planes alone", 300, 6.0f, true);
        const float through[7] = { -6, 0.5f, 0.25f, 1, 0, 0, INFINITY }, inside[7] = { 0.5f, 0.5f, 0.25f, 1, 0, 0, INFINITY }, tangent_free[7] = { -6, 3, 0, 1, 0, 0, INFINITY };
        CHECK(exhaustive(s, through).size() == 3 && exhaustive(s, inside).size() == 2 && exhaustive(s, tangent_free).size() == 1, "sphere crossings: %d %d %d",
              (int)exhaustive(s, through).size(), (int)exhaustive(s, inside).size(), (int)exhaustive(s, tangent_free).size());
        dead_rows(s);
    }
    {   // an empty scene
        Scene s; dead_rows(s);
        const float row[7] = { 0, 0, 0, 1, 0, 0, INFINITY };
        Access A{ s }; Stack st(1); List L(8); rtxhp::Tally w;
        rtxhp::walk(A, st, L, row, 8, true, w);
        CHECK(w.count == 0 && w.held == 0, "an empty scene has no surface");
    }
    // the order rule, and the sorted insert on its own: every permutation prefix of a fixed set ends as the sorted first K
    CHECK(rtxhp::before(1.0f, 5, 2, 1.0f, 5, 3) && rtxhp::before(1.0f, 4, 9, 1.0f, 5, 0) && rtxhp::before(0.5f, 9, 9, 1.0f, 0, 0) && !rtxhp::before(1.0f, 5, 2, 1.0f, 5, 2) && !rtxhp::before(NAN, 0, 0, 1.0f, 0, 0), "the order rule");
    for (int K = 1; K <= 8; K++) for (int trial = 0; trial < 200; trial++) {
        std::vector<Hit> in;
        const int n = 1 + (int)(rnd() * 20.0f);
        for (int i = 0; i < n; i++) in.push_back(Hit{ (float)(int)(rnd() * 6.0f), (int32_t)(rnd() * 3.0f), (int32_t)(rnd() * 3.0f) });
        List L(K); rtxhp::Tally w; w.count = 0; w.held = 0; w.bound = INFINITY;
        for (const Hit & x : in) rtxhp::offer(L, K, true, w, x.t, x.object, x.triangle);
        std::stable_sort(in.begin(), in.end(), [](const Hit & a, const Hit & b) { return rtxhp::before(a.t, a.object, a.triangle, b.t, b.object, b.triangle); });
        CHECK(w.count == n && w.held == (n < K ? n : K), "insert: count %d held %d of %d, K %d", w.count, w.held, n, K);
        for (int j = 0; j < w.held; j++) CHECK(L.h[j].t == in[j].t && L.h[j].object == in[j].object && L.h[j].triangle == in[j].triangle, "insert: entry %d of K %d", j, K);
        CHECK(w.held < K || w.bound == L.h[K - 1].t, "insert: the bound is the K-th hit's t");
    }
    printf("hits_check: %ld rows (%ld with more than 8 hits, most %d), %ld lists of which %ld equal the exhaustive prefix, %ld hits behind a rejected box, deepest stack %d of %d\n",
           rows_checked, rows_over_k, most_hits, lists_total, lists_equal, hits_missed, worst_stack, RTX_MAX_STACK);
    CHECK(rows_over_k > 100, "the generator made too few rows with more than 8 hits (%ld)", rows_over_k);
    CHECK(worst_stack > RTX_MAX_STACK / 2, "the generator never went deep (%d)", worst_stack);
    if (fails) { printf("hits_check: %d FAILED\n", fails); return 1; }
    printf("hits_check: ok\n");
    return 0;
}
