// boxsweep_check.cpp — the walk and the candidate functions of rtx_query_sweep_box (rtx_boxsweep_math.h) against the exhaustive search over
// the same functions, on generated trees, under the host sanitizers (make boxsweep_check).  No GPU, no ROCm.
//   trees      chains, combs, balanced trees and left-deep chains for the BLAS and the TLAS, up to the stack bound of RTX_MAX_STACK entries;
//              duplicated slots; degenerate and NaN triangles; coincident instances with different masks; spheres and planes
//   rows       random oriented boxes flying at the scene, across it and away from it, boxes that start overlapping, zero-extent boxes,
//              unnormalised quaternions, D = +inf, hostile rows (NaN, inf, a zero direction, a negative half extent, a zero quaternion, D <= 0)
//   checked    the walk's t never below the exhaustive t; equal t: the same primitive and axis; a later t only within the header's bound in
//              distance (counted, and rare); no hidden object and no NaN slot in any answer; a row of mask 0 and a hostile row unanswered
//              and not walked; the stack never above rtxnp::stack_need
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <set>
#include <utility>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_boxsweep_math.h"

using rtxnp::P3;

static uint32_t rng_state = 24680u;
static uint32_t rnd_u32() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return (float)rnd_u32() * (1.0f / 16777216.0f); }
static float rnd(float lo, float hi) { return lo + (hi - lo) * rnd(); }
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Mesh { std::vector<rtx_bvh_node> nodes; std::vector<rtx_triangle_hot> hot; int inner_depth = -1; };
struct Scene {
    std::vector<Mesh> meshes; std::vector<rtx_instance> inst; std::vector<rtx_bvh_node> tlas; std::vector<int32_t> tlas_idx;
    std::vector<rtx_sphere> spheres; std::vector<rtx_plane> planes; int tlas_depth = -1;
    std::vector<uint32_t> masks;                                  // instances, spheres, planes: the numbering of RTX_AOV_OBJECT_ID
    int objects() const { return (int)(inst.size() + spheres.size() + planes.size()); }
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
    return b;
}

// a tree over primitive boxes [lo, hi) in the reference node layout; shape 0 chain, 1 comb, 2 balanced, 3 left-deep chain; leaves of <= leaf_max
enum { CHAIN = 0, COMB = 1, BALANCED = 2, LEFT_CHAIN = 3 };      // LEFT_CHAIN: the deep child is the left one, so a box that contains everything holds one sibling per level
static Box build(std::vector<rtx_bvh_node> & nodes, int self, const std::vector<Box> & prims, int lo, int hi, int shape, int leaf_max, int depth, int & inner_depth) {
    Box b = empty_box();
    if (hi - lo <= leaf_max) {
        for (int i = lo; i < hi; i++) merge(b, prims[i]);
        nodes[self].left_or_first = lo; nodes[self].count = hi - lo;
    } else {
        if (depth > inner_depth) inner_depth = depth;
        const int left = (int)nodes.size();
        nodes.push_back(rtx_bvh_node()); nodes.push_back(rtx_bvh_node());
        const int mid = shape == BALANCED ? (lo + hi) / 2 : shape == LEFT_CHAIN ? hi - leaf_max : (shape == CHAIN || (depth & 1)) ? lo + leaf_max : hi - leaf_max;
        const Box l = build(nodes, left, prims, lo, mid, shape, leaf_max, depth + 1, inner_depth);
        const Box r = build(nodes, left + 1, prims, mid, hi, shape, leaf_max, depth + 1, inner_depth);
        merge(b, l); merge(b, r);
        nodes[self].left_or_first = left; nodes[self].count = (int32_t)((uint32_t)(1 + depth % 3) << 30);
    }
    memcpy(nodes[self].aabb_min, b.mn, 12); memcpy(nodes[self].aabb_max, b.mx, 12);
    return b;
}
// n triangles; hostile: every 7th degenerate (a zero edge, or two equal edges), every 11th with a NaN component, every 5th a copy of the slot before it
static Mesh make_mesh(int n, int shape, int leaf_max, bool hostile) {
    Mesh m;
    for (int i = 0; i < n; i++) {
        rtx_triangle_hot t;
        for (int a = 0; a < 3; a++) { t.position_0[a] = rnd(-4.0f, 4.0f); t.position_edge_1[a] = rnd(-1.0f, 1.0f); t.position_edge_2[a] = rnd(-1.0f, 1.0f); }
        if (hostile && i % 7 == 3) for (int a = 0; a < 3; a++) t.position_edge_2[a] = (i & 1) ? 0.0f : t.position_edge_1[a];
        if (hostile && i % 5 == 4 && i > 0) t = m.hot[i - 1];
        m.hot.push_back(t);
    }
    std::vector<Box> prims;
    for (const rtx_triangle_hot & t : m.hot) prims.push_back(tri_box(t));
    if (hostile) for (int i = 0; i < n; i++) if (i % 11 == 6) { if (i & 1) m.hot[i].position_0[i % 3] = NAN; else m.hot[i].position_edge_1[i % 3] = NAN; }      // after the boxes: a pad triangle inside a finite box
    m.nodes.push_back(rtx_bvh_node());
    build(m.nodes, 0, prims, 0, n, shape, leaf_max, 0, m.inner_depth);
    return m;
}
static void identity(float m[16]) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
// rotation about z by `angle` then translation t: world and its inverse, cells[i + 4j] as xform_pos reads them
static rtx_instance make_instance(int blas, float angle, const float t[3]) {
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
    // what the OBJECTS form relies on: every instance in exactly one TLAS leaf
    std::vector<int> seen(s.inst.size(), 0);
    std::vector<int> todo(1, 0);
    while (!todo.empty()) {
        const rtx_bvh_node & nd = s.tlas[todo.back()]; todo.pop_back();
        const int cnt = nd.count & 0x3fffffff;
        if (cnt > 0) for (int i = nd.left_or_first; i < nd.left_or_first + cnt; i++) seen[s.tlas_idx[i]]++;
        else { todo.push_back(nd.left_or_first); todo.push_back(nd.left_or_first + 1); }
    }
    for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == 1, "instance %d is in %d TLAS leaves", (int)i, seen[i]);
}

// the Scene of the walk, with FILTER's predicates over s.masks and one row mask
struct Access {
    const Scene & s; uint32_t row_mask; const Mesh * M = nullptr; long entered = 0;
    bool object_visible(int object) const { return rtxnp::mask_visible(s.masks.at(object), row_mask); }
    bool row_visible() const { return row_mask != 0u; }
    bool sphere_visible(int i) const { return object_visible((int)s.inst.size() + i); }
    bool plane_visible(int i) const { return object_visible((int)(s.inst.size() + s.spheres.size()) + i); }
    bool instance_visible(int slot) const { return object_visible(s.tlas_idx.at(slot)); }
    int instance_count() const { return (int)s.inst.size(); }
    int sphere_count() const { return (int)s.spheres.size(); }
    int plane_count() const { return (int)s.planes.size(); }
    int tlas_nodes() const { return (int)s.tlas.size(); }
    void sphere(int i, P3 & c, float & r2) const { c = rtxnp::ptr3(s.spheres[i].center); r2 = s.spheres[i].radius_squared; }
    void plane(int i, P3 & n, float & d) const { n = rtxnp::ptr3(s.planes[i].normal); d = s.planes[i].distance; }
    static void node(const rtx_bvh_node & nd, P3 & mn, P3 & mx, int & first, int & count) { mn = rtxnp::ptr3(nd.aabb_min); mx = rtxnp::ptr3(nd.aabb_max); first = nd.left_or_first; count = nd.count; }
    void tlas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(s.tlas.at(i), mn, mx, f, c); }
    void blas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(M->nodes.at(i), mn, mx, f, c); }
    int enter(int slot, rtxop::Frame & F, P3 & cd) {
        const int inst = s.tlas_idx.at(slot);
        CHECK(object_visible(inst), "the walk entered hidden instance %d", inst);
        F = rtxop::local_frame(F, s.inst[inst].world_inv); cd = rtxnp::xform_dir(s.inst[inst].world_inv, cd); M = &s.meshes[s.inst[inst].blas_id];
        entered++;
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

// the exhaustive search over the visible set, by the header's functions and order rule
static rtxbs::Answer exhaustive(const Scene & s, Access & A, const float * row) {
    rtxbs::Answer a; rtxbs::clear(a);
    if (!rtxbs::row_is_live(row) || !A.row_visible()) return a;
    const float D = row[6];
    a.t = D;
    const rtxop::Frame W = rtxbs::world_frame(row);
    const P3 d = rtxnp::mk(row[3], row[4], row[5]);
    rtxbs::world_primitives(A, a, W, d, rtxop::to_box(W, d), D);
    for (int k = 0; k < (int)s.inst.size(); k++) {
        if (!A.object_visible(k)) continue;
        const rtxop::Frame F = rtxop::local_frame(W, s.inst[k].world_inv);
        const P3 w = rtxop::to_box(F, rtxnp::xform_dir(s.inst[k].world_inv, d));
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t j = 0; j < M.hot.size(); j++) {
            float t; int axis;
            if (rtxbs::triangle_sweep(F, w, rtxnp::ptr3(M.hot[j].position_0), rtxnp::ptr3(M.hot[j].position_edge_1), rtxnp::ptr3(M.hot[j].position_edge_2), a.t, t, axis)) rtxbs::offer(a, D, t, k, (int32_t)j, axis);
        }
    }
    rtxbs::finish(a);
    return a;
}

static int worst_stack = 0;
static long rows_checked = 0, rows_answered = 0, rows_equal = 0, rows_later = 0, rows_overlap = 0, rows_sphere = 0, rows_plane = 0, axes_seen[16];

static uint32_t pick_row_mask(int i) {
    const int k = i % 8;
    if (k == 0) return 0u;
    if (k < 3) return 1u << (rnd_u32() % 4);
    if (k < 5) { const uint32_t a = rnd_u32() % 4, b = (a + 1 + rnd_u32() % 3) % 4; return (1u << a) | (1u << b); }
    return 0xffffffffu;
}
// row kinds: 0 at the scene from outside, 1 across it from inside, 2 zero extents, 3 axis aligned, 4 unnormalised quaternion, 5 hostile, 6 away from it
static void make_row(float * r, int kind, int i, float reach) {
    for (int a = 0; a < 3; a++) { r[a] = rnd(-reach, reach); r[3 + a] = rnd(-1.0f, 1.0f); r[7 + a] = rnd(0.02f, 0.8f); }
    for (int a = 0; a < 4; a++) r[10 + a] = rnd(-1.0f, 1.0f);
    if (r[10] == 0.0f && r[11] == 0.0f && r[12] == 0.0f && r[13] == 0.0f) r[13] = 1.0f;
    if (r[3] == 0.0f && r[4] == 0.0f && r[5] == 0.0f) r[3] = 1.0f;
    r[6] = (i % 3 == 0) ? INFINITY : rnd(0.5f, 4.0f * reach);
    if (kind == 0 || kind == 6) { for (int a = 0; a < 3; a++) { r[a] = r[3 + a] * -2.0f * reach + rnd(-0.3f, 0.3f) * reach; if (kind == 6) r[3 + a] = -r[3 + a]; } }
    if (kind == 2) { const int z = 1 + i % 7; for (int a = 0; a < 3; a++) if ((z >> a) & 1) r[7 + a] = 0.0f; }
    if (kind == 3) { r[10] = r[11] = r[12] = 0.0f; r[13] = 1.0f; if (i & 1) { r[4] = 0.0f; r[5] = 0.0f; if (r[3] == 0.0f) r[3] = 1.0f; } }
    if (kind == 4) { const float f = (i & 1) ? 1e-12f : 3e12f; for (int a = 0; a < 4; a++) r[10 + a] *= f; }
    if (kind == 5) {
        switch (i % 9) {
            case 0: r[i % 14] = NAN; break;
            case 1: r[(i / 9) % 6] = (i & 2) ? INFINITY : -INFINITY; break;
            case 2: r[7 + i % 3] = -0.25f; break;
            case 3: r[10] = r[11] = r[12] = r[13] = 0.0f; break;
            case 4: r[3] = 0.0f; r[4] = -0.0f; r[5] = 0.0f; break;
            case 5: r[6] = 0.0f; break;
            case 6: r[6] = -3.0f; break;
            case 7: r[7 + i % 3] = INFINITY; break;
            default: r[10] = 3e30f; break;                                      // q.q overflows
        }
    }
}

static void check_scene(const Scene & s, const char * what, int rows, float reach, bool hide_all) {
    int deepest = -1;
    for (const Mesh & m : s.meshes) if (m.inner_depth > deepest) deepest = m.inner_depth;
    const int need = rtxnp::stack_need(s.tlas_depth, deepest);
    CHECK(need <= RTX_MAX_STACK, "%s: the generator exceeded the stack bound (%d)", what, need);
    CHECK((int)s.masks.size() == s.objects(), "%s: one mask per object", what);
    for (int i = 0; i < rows; i++) {
        const uint32_t rm = hide_all ? 16u << (i % 4) : pick_row_mask(i);
        const int kind = i % 16 == 15 ? 5 : (i % 16) % 7 == 5 ? 0 : (i % 16) % 7;
        float row[14];
        make_row(row, kind, i, reach);
        const bool live = rtxbs::row_is_live(row);
        CHECK(live == (kind != 5), "%s row %d kind %d: liveness %d", what, i, kind, (int)live);
        Access E{ s, rm };
        const rtxbs::Answer e = exhaustive(s, E, row);
        Access A{ s, rm }; Stack st(need > 0 ? need : 1);
        rtxbs::Answer w;
        rtxbs::walk(A, st, row, w);
        if (st.high > worst_stack) worst_stack = st.high;
        CHECK(st.high <= need, "%s row %d: stack %d above the stated %d", what, i, st.high, need);
        rows_checked++;
        if (!live || rm == 0u || hide_all) {
            CHECK(w.object == -1 && w.slot == -1 && w.axis == -1 && w.t == INFINITY && A.entered == 0, "%s row %d: a row that sees nothing is answered or was walked", what, i);
            CHECK(e.object == -1 && e.t == INFINITY, "%s row %d: the exhaustive search answers a row that sees nothing", what, i);
            continue;
        }
        CHECK(!(w.t < e.t), "%s row %d: the walk's t %.9g is below the exhaustive %.9g", what, i, w.t, e.t);
        CHECK((w.object < 0) == (w.t == INFINITY) && (w.object < 0) == (w.axis < 0), "%s row %d: a half answer", what, i);
        if (w.object >= 0) {
            rows_answered++;
            CHECK(w.t >= 0.0f && w.t < row[6], "%s row %d: t %.9g outside [0, D)", what, i, w.t);
            CHECK(E.object_visible(w.object), "%s row %d: hidden object %d answers", what, i, w.object);
            CHECK(w.axis != rtxbs::AXIS_OVERLAP || w.t == 0.0f, "%s row %d: t %.9g with axis %d", what, i, w.t, w.axis);
            CHECK((w.slot >= 0) == (w.object < (int)s.inst.size()), "%s row %d: object %d with slot %d", what, i, w.object, w.slot);
            if (w.axis >= 0 && w.axis < 16) axes_seen[w.axis]++;
            if (w.t == 0.0f) rows_overlap++;
            if (w.axis == rtxbs::AXIS_SPHERE) rows_sphere++;
            if (w.axis == rtxbs::AXIS_PLANE) rows_plane++;
            if (w.slot >= 0) {
                const rtx_triangle_hot & t = s.meshes[s.inst[w.object].blas_id].hot[w.slot];
                for (int a = 0; a < 3; a++) CHECK(t.position_0[a] == t.position_0[a] && t.position_edge_1[a] == t.position_edge_1[a] && t.position_edge_2[a] == t.position_edge_2[a], "%s row %d: a NaN slot answers", what, i);
            }
        }
        if (w.t == e.t) { rows_equal++; CHECK(w.object == e.object && w.slot == e.slot && w.axis == e.axis, "%s row %d: equal t %.9g, (%d, %d, %d) against the exhaustive (%d, %d, %d)", what, i, w.t, w.object, w.slot, w.axis, e.object, e.slot, e.axis); }
        else rows_later++;
    }
}

static void random_masks(Scene & s) { s.masks.clear(); for (int k = 0; k < s.objects(); k++) s.masks.push_back(rnd_u32() % 16u); }

int main() {
    const float zero[3] = { 0, 0, 0 };
    // one unmoved instance, chains, combs and left-deep chains up to the stack bound (63 leaves of one slot = inner depth 61, need 62), and a balanced tree
    for (int shape = CHAIN; shape <= LEFT_CHAIN; shape++)
        for (int leaf = 1; leaf <= 4; leaf += 3) {
            Scene s;
            const int n = shape == BALANCED ? 200 : 63 * leaf - (leaf > 1 ? 1 : 0);
            s.meshes.push_back(make_mesh(n, shape, leaf, true));
            s.inst.push_back(make_instance(0, 0.0f, zero));
            make_tlas(s, BALANCED, 1);
            s.masks.assign(1, 0xffffffffu);
            char what[64]; snprintf(what, sizeof what, "shape %d leaf %d", shape, leaf);
            check_scene(s, what, 320, 6.0f, false);
        }
    {   // deep TLAS over deep BLAS at the bound exactly (31 + 33 = 64), random masks
        Scene s;
        s.meshes.push_back(make_mesh(34, CHAIN, 1, false));
        s.meshes.push_back(make_mesh(40, COMB, 2, true));
        for (int k = 0; k < 32; k++) { const float t[3] = { rnd(-8, 8), rnd(-8, 8), rnd(-8, 8) }; s.inst.push_back(make_instance(k % 3 == 2 ? 1 : 0, k % 2 ? rnd(-3, 3) : 0.0f, t)); }
        make_tlas(s, CHAIN, 1);
        CHECK(rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth) == RTX_MAX_STACK, "the deep scene sits at the bound (%d)", rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth));
        random_masks(s);
        check_scene(s, "deep TLAS over deep BLAS", 640, 12.0f, false);
        for (uint32_t & m : s.masks) m &= 15u;
        check_scene(s, "deep TLAS over deep BLAS, everything hidden", 64, 12.0f, true);
    }
    {   // coincident instances with different masks, spheres (one the row starts inside of) and a plane
        Scene s;
        s.meshes.push_back(make_mesh(120, BALANCED, 3, true));
        const float t0[3] = { 1.5f, -0.5f, 0.25f }, t1[3] = { -3.0f, 2.0f, 1.0f }, t2[3] = { 4.0f, 4.0f, -2.0f };
        s.inst.push_back(make_instance(0, 0.7f, t0)); s.inst.push_back(make_instance(0, 0.7f, t0));
        s.inst.push_back(make_instance(0, 0.0f, t1)); s.inst.push_back(make_instance(0, 0.0f, t1));
        s.inst.push_back(make_instance(0, -1.1f, zero));
        for (int k = 0; k < 6; k++) s.inst.push_back(make_instance(0, 0.3f * k, t2));
        make_tlas(s, COMB, 3);
        rtx_sphere sp; memset(&sp, 0, sizeof sp); sp.center[0] = 2; sp.center[1] = 3; sp.center[2] = -1; sp.radius_squared = 2.25f; sp.radius_inv = 1.0f / 1.5f;
        s.spheres.push_back(sp);
        sp.center[0] = 0; sp.center[1] = 0; sp.center[2] = 0; sp.radius_squared = 900.0f; sp.radius_inv = 1.0f / 30.0f;      // everything starts inside this one
        s.spheres.push_back(sp);
        rtx_plane pl; memset(&pl, 0, sizeof pl); pl.normal[1] = 1.0f; pl.distance = 12.0f; pl.u_axis[0] = 1.0f; pl.v_axis[2] = 1.0f;
        s.planes.push_back(pl);
        const uint32_t masks[] = { 1, 2, 4, 8, 15, 8, 8, 8, 8, 8, 8, /* spheres */ 3, 12, /* plane */ 6 };
        s.masks.assign(masks, masks + sizeof masks / sizeof masks[0]);
        check_scene(s, "coincident instances, spheres, a plane", 1280, 8.0f, false);
        for (uint32_t & m : s.masks) m = 0u;
        check_scene(s, "a table that hides everything", 64, 8.0f, false);
    }
    long cross = 0;
    for (int k = 4; k < 13; k++) cross += axes_seen[k];
    printf("boxsweep_check: %ld rows, %ld answered (%ld at t = 0, %ld by a sphere, %ld by a plane, %ld by a cross axis), %ld equal to the exhaustive search, %ld later, deepest stack %d of %d\n",
           rows_checked, rows_answered, rows_overlap, rows_sphere, rows_plane, cross, rows_equal, rows_later, worst_stack, RTX_MAX_STACK);
    CHECK(rows_later * 200 <= rows_checked, "the walk is later than the exhaustive search on %ld of %ld rows: the slab test is not conservative", rows_later, rows_checked);
    CHECK(rows_answered > rows_checked / 8 && rows_overlap > 50 && rows_sphere > 20 && rows_plane > 20 && cross > 50 && worst_stack >= 62, "too little happened for the check to mean anything");
    if (fails) { printf("boxsweep_check: %d FAILED\n", fails); return 1; }
    printf("boxsweep_check: ok\n");
    return 0;
}
