// nearest_check.cpp — the walk of rtx_query_nearest (rtx_nearest_math.h) against the exhaustive search over the same candidate functions, on
// generated trees, under the host sanitizers (make nearest_check).  No GPU, no ROCm.
//   trees      chains (every inner node = one leaf + the rest), combs (the leaf alternates sides) and balanced trees, for the BLAS and the
//              TLAS, up to the stack bound of RTX_MAX_STACK entries; leaves of 1 .. 4 slots
//   triangles  random, duplicated slots, degenerate (zero edge, parallel edges) and NaN triangles
//   instances  translated, rotated, and coincident pairs (same mesh, same matrix)
//   checked    walk distance >= exhaustive distance; walk distance <= exhaustive distance + rtxnp::distance_bound of the exhaustive winner;
//              the stack never above rtxnp::stack_need; spheres and planes exactly; hostile rows get the no-answer record
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_nearest_math.h"

using rtxnp::P3;

static uint32_t rng_state = 12345u;
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

// a tree over primitive boxes [lo, hi) of `prims` in the reference node layout; shape 0 chain, 1 comb, 2 balanced; leaves of <= leaf_max
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
        int mid = shape == BALANCED ? (lo + hi) / 2 : (shape == CHAIN || (depth & 1)) ? lo + leaf_max : hi - leaf_max;
        const Box l = build(nodes, left, prims, lo, mid, shape, leaf_max, depth + 1, inner_depth);
        const Box r = build(nodes, left + 1, prims, mid, hi, shape, leaf_max, depth + 1, inner_depth);
        merge(b, l); merge(b, r);
        nodes[self].left_or_first = left; nodes[self].count = (int32_t)((uint32_t)(1 + depth % 3) << 30);
    }
    memcpy(nodes[self].aabb_min, b.mn, 12); memcpy(nodes[self].aabb_max, b.mx, 12);
    return b;
}

static rtx_triangle_hot random_triangle(float spread, float size) {
    rtx_triangle_hot t;
    for (int a = 0; a < 3; a++) { t.position_0[a] = rnd(-spread, spread); t.position_edge_1[a] = rnd(-size, size); t.position_edge_2[a] = rnd(-size, size); }
    return t;
}
static Mesh make_mesh(int n, int shape, int leaf_max, bool hostile) {
    Mesh m;
    for (int i = 0; i < n; i++) {
        rtx_triangle_hot t = random_triangle(4.0f, 1.0f);
        if (hostile) {
            const int k = i % 7;
            if (k == 1 && i > 0) t = m.hot[i - 1];                                                     // a duplicated slot
            if (k == 2) for (int a = 0; a < 3; a++) t.position_edge_1[a] = 0.0f;                       // a zero edge
            if (k == 3) for (int a = 0; a < 3; a++) t.position_edge_2[a] = 2.0f * t.position_edge_1[a]; // parallel edges
            if (k == 4) for (int a = 0; a < 3; a++) t.position_edge_1[a] = t.position_edge_2[a] = 0.0f; // a point
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
// rotation about z by `angle` then translation t: world and its inverse, cells[i + 4j] as xform_pos reads them (row j at 4j)
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
// the world box of an instance: its mesh's root box through `world`, all eight corners (its rounding is the W term of the bound)
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
    int sphere_count() const { return (int)s.spheres.size(); }
    int plane_count() const { return (int)s.planes.size(); }
    int tlas_nodes() const { return (int)s.tlas.size(); }
    void sphere(int i, P3 & c, float & r2) const { c = rtxnp::ptr3(s.spheres[i].center); r2 = s.spheres[i].radius_squared; }
    void plane(int i, P3 & n, float & d) const { n = rtxnp::ptr3(s.planes[i].normal); d = s.planes[i].distance; }
    static void node(const rtx_bvh_node & nd, P3 & mn, P3 & mx, int & first, int & count) { mn = rtxnp::ptr3(nd.aabb_min); mx = rtxnp::ptr3(nd.aabb_max); first = nd.left_or_first; count = nd.count; }
    void tlas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(s.tlas.at(i), mn, mx, f, c); }
    void blas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(M->nodes.at(i), mn, mx, f, c); }
    int enter(int slot, P3 p, P3 & pl) { const int inst = s.tlas_idx.at(slot); pl = rtxnp::xform_pos(s.inst[inst].world_inv, p); M = &s.meshes[s.inst[inst].blas_id]; return inst; }
    void triangle(int i, P3 & p0, P3 & e1, P3 & e2) const { const rtx_triangle_hot & t = M->hot.at(i); p0 = rtxnp::ptr3(t.position_0); e1 = rtxnp::ptr3(t.position_edge_1); e2 = rtxnp::ptr3(t.position_edge_2); }
};
struct Stack {
    std::vector<int> node; std::vector<float> d2; int high = 0;
    explicit Stack(int cap) : node(cap), d2(cap) {}
    void push(int sp, int n, float d) { node.at(sp) = n; d2.at(sp) = d; if (sp + 1 > high) high = sp + 1; }      // at(): beyond the stated count is a failure
    void pop(int sp, int & n, float & d) const { n = node.at(sp); d = d2.at(sp); }
};

static rtxnp::Answer exhaustive(const Scene & s, const float * row) {
    rtxnp::Answer a; a.kind = rtxnp::KIND_NONE; a.object = a.slot = -1; a.u = a.v = 0.0f; a.d2 = INFINITY;
    if (!rtxnp::row_is_live(row)) return a;
    const P3 p = rtxnp::mk(row[0], row[1], row[2]);
    a.d2 = row[3] * row[3];
    for (size_t k = 0; k < s.spheres.size(); k++) rtxnp::offer(a, rtxnp::sphere_d2(p, rtxnp::ptr3(s.spheres[k].center), s.spheres[k].radius_squared), rtxnp::KIND_SPHERE, (int)k, -1, 0, 0);
    for (size_t k = 0; k < s.planes.size(); k++) rtxnp::offer(a, rtxnp::plane_d2(p, rtxnp::ptr3(s.planes[k].normal), s.planes[k].distance), rtxnp::KIND_PLANE, (int)k, -1, 0, 0);
    for (size_t k = 0; k < s.inst.size(); k++) {
        const P3 pl = rtxnp::xform_pos(s.inst[k].world_inv, p);
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t t = 0; t < M.hot.size(); t++) {
            float u, v;
            const float d2 = rtxnp::triangle_d2(rtxnp::sub(pl, rtxnp::ptr3(M.hot[t].position_0)), rtxnp::ptr3(M.hot[t].position_edge_1), rtxnp::ptr3(M.hot[t].position_edge_2), u, v);
            rtxnp::offer(a, d2, rtxnp::KIND_TRI, (int)k, (int)t, u, v);
        }
    }
    return a;
}
static double len(const float v[3]) { return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

static double worst_ratio = 0.0;
static int worst_stack = 0;
static long rows_checked = 0;

static void check_scene(const Scene & s, const char * what, int points, float reach) {
    int deepest = -1;
    for (const Mesh & m : s.meshes) if (m.inner_depth > deepest) deepest = m.inner_depth;
    const int need = rtxnp::stack_need(s.tlas_depth, deepest);
    CHECK(need <= RTX_MAX_STACK, "%s: the generator exceeded the stack bound (%d)", what, need);
    for (int i = 0; i < points; i++) {
        float row[4] = { rnd(-reach, reach), rnd(-reach, reach), rnd(-reach, reach), INFINITY };
        if (i % 5 == 1) row[3] = rnd(0.01f, reach);
        if (i % 11 == 3 && !s.meshes.empty()) {                            // exactly on a vertex of mesh 0 (local space: a tie between its neighbours when the instance is unmoved)
            const rtx_triangle_hot & t = s.meshes[0].hot[i % s.meshes[0].hot.size()];
            if (t.position_0[0] == t.position_0[0] && t.position_0[1] == t.position_0[1] && t.position_0[2] == t.position_0[2]) memcpy(row, t.position_0, 12);
        }
        Access A{ s }; Stack st(need > 0 ? need : 1);
        rtxnp::Answer w;
        rtxnp::walk(A, st, row, w);
        const rtxnp::Answer e = exhaustive(s, row);
        rows_checked++;
        if (st.high > worst_stack) worst_stack = st.high;
        CHECK(st.high <= need, "%s: stack %d above the stated %d", what, st.high, need);
        CHECK((w.kind == rtxnp::KIND_NONE) == (e.kind == rtxnp::KIND_NONE) || e.kind == rtxnp::KIND_TRI, "%s row %d: the walk answers %d, the exhaustive search %d", what, i, w.kind, e.kind);
        if (e.kind == rtxnp::KIND_NONE) { CHECK(w.kind == rtxnp::KIND_NONE && w.d2 == e.d2, "%s row %d: an answer nothing justifies", what, i); continue; }
        const float dw = w.kind == rtxnp::KIND_NONE ? INFINITY : rtxnp::root(w.d2), de = rtxnp::root(e.d2);
        CHECK(dw >= de, "%s row %d: walk %.9g below exhaustive %.9g", what, i, dw, de);
        if (e.kind != rtxnp::KIND_TRI) { CHECK(w.kind == e.kind && w.object == e.object && w.d2 == e.d2, "%s row %d: spheres and planes are never pruned", what, i); continue; }
        const rtx_instance & I = s.inst[e.object];
        const rtx_triangle_hot & t = s.meshes[I.blas_id].hot[e.slot];
        const P3 p = rtxnp::mk(row[0], row[1], row[2]), pl = rtxnp::xform_pos(I.world_inv, p);
        const float ap[3] = { pl.x - t.position_0[0], pl.y - t.position_0[1], pl.z - t.position_0[2] }, pw[3] = { p.x, p.y, p.z }, plv[3] = { pl.x, pl.y, pl.z };
        const double S = len(ap) + len(t.position_edge_1) + len(t.position_edge_2);
        bool ident = true; { float id[16]; identity(id); ident = memcmp(id, I.world_inv, 64) == 0; }
        const double W = ident ? 0.0 : len(pw) + len(plv);
        const double bound = rtxnp::distance_bound((float)S, (float)W);
        // a maximum distance cuts the walk's answer off: the exhaustive winner lies within the bound of it then
        const double excess = (w.kind == rtxnp::KIND_NONE ? (double)row[3] : (double)dw) - (double)de;
        CHECK(excess <= bound, "%s row %d: walk %.9g exceeds exhaustive %.9g by %.3g, bound %.3g", what, i, dw, de, excess, bound);
        if (excess > 0 && excess / bound > worst_ratio) worst_ratio = excess / bound;
    }
}

static void hostile_rows(const Scene & s) {
    const float bad[][4] = { { NAN, 0, 0, 1 }, { 0, INFINITY, 0, 1 }, { 0, 0, -INFINITY, INFINITY }, { 0, 0, 0, NAN }, { 0, 0, 0, 0 }, { 0, 0, 0, -0.0f }, { 0, 0, 0, -1 },
                             { 1e30f, 1e30f, 1e30f, INFINITY }, { 3e38f, -3e38f, 3e38f, INFINITY }, { 0, 0, 0, 1e-30f }, { 0, 0, 0, -INFINITY } };
    for (const float * row : bad) {
        Access A{ s }; Stack st(RTX_MAX_STACK);
        rtxnp::Answer w;
        rtxnp::walk(A, st, row, w);
        CHECK(w.kind == rtxnp::KIND_NONE && w.object == -1 && w.slot == -1 && w.u == 0.0f && w.v == 0.0f, "hostile row (%g %g %g %g) got an answer of kind %d", row[0], row[1], row[2], row[3], w.kind);
        rows_checked++;
    }
    const float denormal[4] = { 1e-42f, -1e-42f, 0, INFINITY };           // a legal point
    Access A{ s }; Stack st(RTX_MAX_STACK); rtxnp::Answer w;
    rtxnp::walk(A, st, denormal, w);
    CHECK(w.kind != rtxnp::KIND_NONE || (s.inst.empty() && s.spheres.empty() && s.planes.empty()), "a denormal point is a point");
}

int main() {
    const float zero[3] = { 0, 0, 0 };
    // one instance, every tree shape and leaf size; chains and combs up to the stack bound: 63 leaves of one slot = inner depth 61, need 62
    for (int shape = CHAIN; shape <= BALANCED; shape++)
        for (int leaf = 1; leaf <= 4; leaf++)
            for (int hostile = 0; hostile < 2; hostile++) {
                Scene s;
                const int n = shape == BALANCED ? 200 : 63 * leaf - (leaf > 1 ? 1 : 0);
                s.meshes.push_back(make_mesh(n, shape, leaf, hostile != 0));
                s.inst.push_back(make_instance(0, 0.0f, zero));
                make_tlas(s, BALANCED, 1);
                char what[64]; snprintf(what, sizeof what, "shape %d leaf %d hostile %d", shape, leaf, hostile);
                check_scene(s, what, 400, 6.0f);
            }
    {   // deep TLAS and deep BLAS together, at the bound exactly: a chain of 32 instances (inner depth 30) over a chain mesh of 34 leaves (32): need 31 + 33 = 64
        Scene s;
        s.meshes.push_back(make_mesh(34, CHAIN, 1, false));
        s.meshes.push_back(make_mesh(40, COMB, 2, true));
        for (int k = 0; k < 32; k++) { const float t[3] = { rnd(-8, 8), rnd(-8, 8), rnd(-8, 8) }; s.inst.push_back(make_instance(k % 3 == 2 ? 1 : 0, k % 2 ? rnd(-3, 3) : 0.0f, t)); }
        make_tlas(s, CHAIN, 1);
        CHECK(rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth) == RTX_MAX_STACK, "the deep scene sits at the bound (%d)", rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth));
        check_scene(s, "deep TLAS over deep BLAS", 600, 14.0f);
        hostile_rows(s);
    }
    {   // coincident instances, spheres and planes, TLAS leaves of several instances
        Scene s;
        s.meshes.push_back(make_mesh(120, BALANCED, 3, true));
        const float t0[3] = { 1.5f, -0.5f, 0.25f }, t1[3] = { -3.0f, 2.0f, 1.0f };
        s.inst.push_back(make_instance(0, 0.7f, t0)); s.inst.push_back(make_instance(0, 0.7f, t0));      // the same mesh twice in one place
        s.inst.push_back(make_instance(0, 0.0f, t1)); s.inst.push_back(make_instance(0, 0.0f, t1));
        s.inst.push_back(make_instance(0, -1.1f, zero));
        make_tlas(s, COMB, 2);
        rtx_sphere sp; memset(&sp, 0, sizeof sp); sp.center[0] = 2; sp.center[1] = 3; sp.center[2] = -1; sp.radius_squared = 2.25f; sp.radius_inv = 1.0f / 1.5f;
        s.spheres.push_back(sp); s.spheres.push_back(sp);
        rtx_plane pl; memset(&pl, 0, sizeof pl); pl.normal[1] = 1.0f; pl.distance = 7.0f; pl.u_axis[0] = 1.0f; pl.v_axis[2] = 1.0f;
        s.planes.push_back(pl);
        check_scene(s, "coincident instances, spheres, planes", 1500, 9.0f);
        hostile_rows(s);
        const float centre[4] = { 2, 3, -1, INFINITY };                  // a sphere's centre: direction (0, 1, 0)
        P3 point, normal; float tu, tv;
        rtxnp::sphere_outputs(rtxnp::mk(centre[0], centre[1], centre[2]), rtxnp::ptr3(sp.center), sp.radius_squared, point, normal, tu, tv);
        CHECK(normal.x == 0.0f && normal.y == 1.0f && normal.z == 0.0f && point.y == 4.5f, "the centre of a sphere answers straight up");
    }
    {   // no TLAS at all, and an empty scene
        Scene s; hostile_rows(s);
        const float row[4] = { 0, 0, 0, INFINITY };
        Access A{ s }; Stack st(1); rtxnp::Answer w;
        rtxnp::walk(A, st, row, w);
        CHECK(w.kind == rtxnp::KIND_NONE, "an empty scene has no surface");
    }
    printf("nearest_check: %ld rows, deepest stack %d of %d, worst excess / bound %.4f\n", rows_checked, worst_stack, RTX_MAX_STACK, worst_ratio);
    if (fails) { printf("nearest_check: %d FAILED\n", fails); return 1; }
    printf("nearest_check: ok\n");
    return 0;
}
