// sweep_check.cpp — the walk of rtx_query_sweep (rtx_sweep_math.h) against the exhaustive search over the same candidate functions, on
// generated trees, under the host sanitizers (make sweep_check).  No GPU, no ROCm.
//   trees      chains, combs and balanced trees, for the BLAS and the TLAS, up to the stack bound of RTX_MAX_STACK entries; leaves of 1 .. 4 slots
//   triangles  random, duplicated slots, degenerate (zero edge, parallel edges, a point) and NaN triangles
//   instances  translated, rotated, and coincident pairs (same mesh, same matrix); spheres (from outside and from inside) and planes
//   checked    walk t >= exhaustive t, and the SAME answer (t, weights, primitive) under an unmoved instance, where the box tests' slack is
//              conservative against the computed candidates; a returned triangle contact within rtxsp::sweep_bound of r in double precision;
//              the stack never above rtxnp::stack_need; hostile rows get the no-answer record
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_sweep_math.h"

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

static rtxsp::Answer exhaustive(const Scene & s, const float * row) {
    rtxsp::Answer a; rtxsp::clear(a);
    if (!rtxsp::row_is_live(row)) return a;
    const P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
    a.t = row[6];
    Access A{ s };
    rtxsp::world_primitives(A, a, o, d, row[6], row[7]);
    for (size_t k = 0; k < s.inst.size(); k++) {
        const P3 co = rtxnp::xform_pos(s.inst[k].world_inv, o), cd = rtxnp::xform_dir(s.inst[k].world_inv, d);
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t j = 0; j < M.hot.size(); j++) {
            float t, u, v, d20;
            if (rtxsp::triangle_sweep(rtxnp::ptr3(M.hot[j].position_0), rtxnp::ptr3(M.hot[j].position_edge_1), rtxnp::ptr3(M.hot[j].position_edge_2), co, cd, row[7], a.t, t, u, v, d20))
                rtxsp::offer(a, row[6], t, d20, rtxnp::KIND_TRI, (int)k, (int)j, u, v);
        }
    }
    return a;
}

// the distance from p to triangle (a, b, c) in double precision: clamped projections onto the three edges, and the face where p is above it
struct D3 { double x, y, z; };
static D3 dsub(D3 a, D3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
static double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 dcross(D3 a, D3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
static double seg_distance(D3 p, D3 a, D3 e) {
    const double ee = ddot(e, e);
    double t = ee > 0 ? ddot(dsub(p, a), e) / ee : 0.0;
    t = t < 0 ? 0 : t > 1 ? 1 : t;
    const D3 r = { p.x - (a.x + t * e.x), p.y - (a.y + t * e.y), p.z - (a.z + t * e.z) };
    return sqrt(ddot(r, r));
}
static double tri_distance(D3 p, D3 a, D3 e1, D3 e2) {
    const D3 b = { a.x + e1.x, a.y + e1.y, a.z + e1.z };
    double best = fmin(fmin(seg_distance(p, a, e1), seg_distance(p, a, e2)), seg_distance(p, b, dsub(e2, e1)));
    const D3 n = dcross(e1, e2), ap = dsub(p, a);
    const double nn = ddot(n, n);
    if (nn > 0) {
        const double u = ddot(dcross(ap, e2), n) / nn, v = ddot(dcross(e1, ap), n) / nn;
        if (u >= 0 && v >= 0 && u + v <= 1) best = fmin(best, fabs(ddot(ap, n)) / sqrt(nn));
    }
    return best;
}
static double len(const float v[3]) { return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }
static D3 d3(const float v[3]) { return { v[0], v[1], v[2] }; }

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }      // a degenerate triangle's d20 is a NaN

static double worst_ratio = 0.0;
static int worst_stack = 0;
static long rows_checked = 0, rows_later = 0, rows_hit = 0;

static void check_scene(const Scene & s, const char * what, int rows, float reach, bool exact) {
    int deepest = -1;
    for (const Mesh & m : s.meshes) if (m.inner_depth > deepest) deepest = m.inner_depth;
    const int need = rtxnp::stack_need(s.tlas_depth, deepest);
    CHECK(need <= RTX_MAX_STACK, "%s: the generator exceeded the stack bound (%d)", what, need);
    for (int i = 0; i < rows; i++) {
        float row[8] = { rnd(-reach, reach), rnd(-reach, reach), rnd(-reach, reach), 0, 0, 0, INFINITY, 0 };
        const float speed = i % 3 == 0 ? 0.05f : i % 3 == 1 ? 1.0f : 7.0f;
        for (int a = 0; a < 3; a++) row[3 + a] = (rnd(-4.0f, 4.0f) - row[a]) * speed * 0.2f;      // towards the middle of the scene, roughly
        row[7] = i % 4 == 0 ? rnd(0.5f, 1.5f) : i % 4 == 1 ? rnd(0.001f, 0.01f) : rnd(0.01f, 0.3f);
        if (i % 5 == 1) row[6] = rnd(0.01f, 2.0f) / speed;
        if (i % 13 == 5) row[3 + i % 3] = 0.0f;                            // an axis-parallel motion: infinite inverse components
        Access A{ s }; Stack st(need > 0 ? need : 1);
        rtxsp::Answer w;
        rtxsp::walk(A, st, row, w);
        const rtxsp::Answer e = exhaustive(s, row);
        rows_checked++;
        if (st.high > worst_stack) worst_stack = st.high;
        CHECK(st.high <= need, "%s: stack %d above the stated %d", what, st.high, need);
        const float tw = w.kind == rtxnp::KIND_NONE ? INFINITY : w.t, te = e.kind == rtxnp::KIND_NONE ? INFINITY : e.t;
        CHECK(tw >= te, "%s row %d: walk %.9g before exhaustive %.9g", what, i, tw, te);
        if (tw > te) rows_later++;
        if (exact) CHECK(tw == te && w.kind == e.kind && w.object == e.object && same_bits(w.u, e.u) && same_bits(w.v, e.v) && (same_bits(w.d20, e.d20) || w.kind == rtxnp::KIND_NONE),
                         "%s row %d: walk (%.9g kind %d slot %d) is not the exhaustive answer (%.9g kind %d slot %d)", what, i, tw, w.kind, w.slot, te, e.kind, e.slot);
        if (e.kind != rtxnp::KIND_TRI && e.kind != rtxnp::KIND_NONE) CHECK(w.kind == e.kind && w.object == e.object && w.t == e.t, "%s row %d: spheres and planes are never pruned", what, i);
        if (w.kind != rtxnp::KIND_NONE) { CHECK(w.t >= 0.0f && w.t < row[6], "%s row %d: t %.9g outside [0, D)", what, i, w.t); rows_hit++; }
        if (w.kind != rtxnp::KIND_TRI) continue;
        const rtx_instance & I = s.inst[w.object];
        const rtx_triangle_hot & t = s.meshes[I.blas_id].hot[w.slot];
        const P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
        const P3 co = rtxnp::xform_pos(I.world_inv, o), cd = rtxnp::xform_dir(I.world_inv, d);
        const float ap[3] = { co.x - t.position_0[0], co.y - t.position_0[1], co.z - t.position_0[2] }, ow[3] = { o.x, o.y, o.z }, ol[3] = { co.x, co.y, co.z }, dl[3] = { cd.x, cd.y, cd.z };
        const double S = len(ap) + len(t.position_edge_1) + len(t.position_edge_2);
        bool ident = true; { float id[16]; identity(id); ident = memcmp(id, I.world_inv, 64) == 0; }
        const double W = ident ? 0.0 : len(ow) + len(ol);
        const double bound = rtxsp::sweep_bound((float)S, (float)W, (float)(w.t * len(dl)), row[7]);
        const D3 c = { co.x + (double)w.t * cd.x, co.y + (double)w.t * cd.y, co.z + (double)w.t * cd.z };
        const double dist = tri_distance(c, d3(t.position_0), d3(t.position_edge_1), d3(t.position_edge_2));
        const double kappa = len(t.position_edge_1) * len(t.position_edge_2) / sqrt(ddot(dcross(d3(t.position_edge_1), d3(t.position_edge_2)), dcross(d3(t.position_edge_1), d3(t.position_edge_2))));
        if (!(kappa <= 4.0)) continue;                                     // slivers and degenerate triangles are outside the bound (ACCURACY, face)
        const double err = w.t == 0.0f ? fmax(0.0, dist - row[7]) : fabs(dist - row[7]);
        CHECK(err <= bound, "%s row %d: contact at distance %.9g, r %.9g, bound %.3g", what, i, dist, (double)row[7], bound);
        if (err / bound > worst_ratio) worst_ratio = err / bound;
    }
}

static void hostile_rows(const Scene & s) {
    const float bad[][8] = { { NAN, 0, 0, 0, 0, 1, 1, 1 }, { 0, INFINITY, 0, 0, 0, 1, 1, 1 }, { 0, 0, 0, NAN, 0, 1, 1, 1 }, { 0, 0, 0, 0, -INFINITY, 1, 1, 1 }, { 0, 0, 0, 0, 0, 0, 1, 1 },
                             { 0, 0, 0, -0.0f, 0, -0.0f, 1, 1 }, { 0, 0, 0, 0, 0, 1, NAN, 1 }, { 0, 0, 0, 0, 0, 1, 0, 1 }, { 0, 0, 0, 0, 0, 1, -1, 1 }, { 0, 0, 0, 0, 0, 1, -INFINITY, 1 },
                             { 0, 0, 0, 0, 0, 1, 1, 0 }, { 0, 0, 0, 0, 0, 1, 1, -0.0f }, { 0, 0, 0, 0, 0, 1, 1, -1 }, { 0, 0, 0, 0, 0, 1, 1, NAN }, { 0, 0, 0, 0, 0, 1, 1, INFINITY } };
    for (const float * row : bad) {
        Access A{ s }; Stack st(RTX_MAX_STACK);
        rtxsp::Answer w;
        rtxsp::walk(A, st, row, w);
        CHECK(w.kind == rtxnp::KIND_NONE && w.object == -1 && w.slot == -1 && w.u == 0.0f && w.v == 0.0f && st.high == 0, "a hostile row got an answer of kind %d", w.kind);
        rows_checked++;
    }
    const float live[][8] = { { 1e-42f, -1e-42f, 0, 0, 0, 1e-42f, 1e6f, 0.1f }, { 1e30f, 1e30f, 1e30f, -1, -1, -1, INFINITY, 0.5f }, { 3e38f, -3e38f, 3e38f, 1, 0, 0, INFINITY, 1e-30f },
                              { 0, 0, 0, 3e38f, 3e38f, 3e38f, INFINITY, 0.25f }, { 0, 0, 0, 1e-45f, 0, 0, INFINITY, 3e38f } };
    for (const float * row : live) {                                       // legal rows at the edge of fp32: whatever they answer, the walk stays in bounds
        Access A{ s }; Stack st(RTX_MAX_STACK);
        rtxsp::Answer w;
        rtxsp::walk(A, st, row, w);
        CHECK(w.kind == rtxnp::KIND_NONE || (w.t >= 0.0f && w.t < row[6]), "a row at the edge of fp32 answers t %.9g", w.t);
        rows_checked++;
    }
}

int main() {
    const float zero[3] = { 0, 0, 0 };
    // one unmoved instance, every tree shape and leaf size; chains and combs up to the stack bound: 63 leaves of one slot = inner depth 61, need 62
    for (int shape = CHAIN; shape <= BALANCED; shape++)
        for (int leaf = 1; leaf <= 4; leaf++)
            for (int hostile = 0; hostile < 2; hostile++) {
                Scene s;
                const int n = shape == BALANCED ? 200 : 63 * leaf - (leaf > 1 ? 1 : 0);
                s.meshes.push_back(make_mesh(n, shape, leaf, hostile != 0));
                s.inst.push_back(make_instance(0, 0.0f, zero));
                make_tlas(s, BALANCED, 1);
                char what[64]; snprintf(what, sizeof what, "shape %d leaf %d hostile %d", shape, leaf, hostile);
                check_scene(s, what, 400, 9.0f, true);
            }
    {   // deep TLAS and deep BLAS together, at the bound exactly: a chain of 32 instances (inner depth 30) over a chain mesh of 34 leaves (32): need 31 + 33 = 64
        Scene s;
        s.meshes.push_back(make_mesh(34, CHAIN, 1, false));
        s.meshes.push_back(make_mesh(40, COMB, 2, true));
        for (int k = 0; k < 32; k++) { const float t[3] = { rnd(-8, 8), rnd(-8, 8), rnd(-8, 8) }; s.inst.push_back(make_instance(k % 3 == 2 ? 1 : 0, k % 2 ? rnd(-3, 3) : 0.0f, t)); }
        make_tlas(s, CHAIN, 1);
        CHECK(rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth) == RTX_MAX_STACK, "the deep scene sits at the bound (%d)", rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth));
        check_scene(s, "deep TLAS over deep BLAS", 600, 16.0f, false);
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
        sp.center[0] = 0; sp.center[1] = 0; sp.center[2] = 0; sp.radius_squared = 400.0f; sp.radius_inv = 0.05f;      // everything happens inside this one
        s.spheres.push_back(sp);
        rtx_plane pl; memset(&pl, 0, sizeof pl); pl.normal[1] = 1.0f; pl.distance = 7.0f; pl.u_axis[0] = 1.0f; pl.v_axis[2] = 1.0f;
        s.planes.push_back(pl);
        check_scene(s, "coincident instances, spheres, planes", 1500, 9.0f, false);
        hostile_rows(s);
    }
    {   // no TLAS at all, and an empty scene
        Scene s; hostile_rows(s);
        const float row[8] = { 0, 0, 0, 0, 0, 1, INFINITY, 1 };
        Access A{ s }; Stack st(1); rtxsp::Answer w;
        rtxsp::walk(A, st, row, w);
        CHECK(w.kind == rtxnp::KIND_NONE, "an empty scene has no surface");
    }
    printf("sweep_check: %ld rows, %ld answered, %ld with a later walk, deepest stack %d of %d, worst contact error / bound %.4f\n", rows_checked, rows_hit, rows_later, worst_stack, RTX_MAX_STACK, worst_ratio);
    CHECK(rows_hit > rows_checked / 4, "too few rows answered for the check to mean anything");
    if (fails) { printf("sweep_check: %d FAILED\n", fails); return 1; }
    printf("sweep_check: ok\n");
    return 0;
}
