// mask_check.cpp — the three filtered walks (FILTER of rtx_nearest_math.h, rtx_hits_math.h, rtx_sweep_math.h) against the filtered exhaustive
// searches over the same candidate functions, on generated trees, under the host sanitizers (make mask_check).  No GPU, no ROCm.
//   trees      chains, combs and balanced trees for the BLAS and the TLAS, up to the stack bound of RTX_MAX_STACK entries; TLAS leaves of 1 .. 3
//   masks      random object masks over 4 bits (0 included); coincident instances with different masks; TLAS leaves whose instances are all
//              hidden from a row; a table that hides everything; row masks 0, one bit, two bits, all ones
//   checked    over the VISIBLE set: nearest never nearer and farther by at most rtxnp::distance_bound of the exhaustive winner; every listed hit
//              a hit of the exhaustive search with the same bits, in order, the count never above; the sweep never earlier, spheres and
//              planes exactly; the stack never above rtxnp::stack_need; no answer names a hidden object; a row of mask 0 is not walked
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_sweep_math.h"

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

// a tree over primitive boxes [lo, hi) in the reference node layout; shape 0 chain, 1 comb, 2 balanced; leaves of <= leaf_max
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
static Mesh make_mesh(int n, int shape, int leaf_max) {
    Mesh m;
    for (int i = 0; i < n; i++) {
        rtx_triangle_hot t;
        for (int a = 0; a < 3; a++) { t.position_0[a] = rnd(-4.0f, 4.0f); t.position_edge_1[a] = rnd(-1.0f, 1.0f); t.position_edge_2[a] = rnd(-1.0f, 1.0f); }
        m.hot.push_back(t);
    }
    std::vector<Box> prims;
    for (const rtx_triangle_hot & t : m.hot) prims.push_back(tri_box(t));
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
}

// the Scene of all three walks, with FILTER's predicates over s.masks and one row mask
struct Access {
    const Scene & s; uint32_t row_mask; const Mesh * M = nullptr; mutable long hidden_skipped = 0;
    bool object_visible(int object) const { return rtxnp::mask_visible(s.masks.at(object), row_mask); }
    bool row_visible() const { return row_mask != 0u; }
    bool sphere_visible(int i) const { return object_visible((int)s.inst.size() + i); }
    bool plane_visible(int i) const { return object_visible((int)(s.inst.size() + s.spheres.size()) + i); }
    bool instance_visible(int slot) const { const bool v = object_visible(s.tlas_idx.at(slot)); if (!v) hidden_skipped++; return v; }
    int instance_count() const { return (int)s.inst.size(); }
    int sphere_count() const { return (int)s.spheres.size(); }
    int plane_count() const { return (int)s.planes.size(); }
    int tlas_nodes() const { return (int)s.tlas.size(); }
    void sphere(int i, P3 & c, float & r2) const { c = rtxnp::ptr3(s.spheres[i].center); r2 = s.spheres[i].radius_squared; }
    void plane(int i, P3 & n, float & d) const { n = rtxnp::ptr3(s.planes[i].normal); d = s.planes[i].distance; }
    static void node(const rtx_bvh_node & nd, P3 & mn, P3 & mx, int & first, int & count) { mn = rtxnp::ptr3(nd.aabb_min); mx = rtxnp::ptr3(nd.aabb_max); first = nd.left_or_first; count = nd.count; }
    void tlas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(s.tlas.at(i), mn, mx, f, c); }
    void blas_node(int i, P3 & mn, P3 & mx, int & f, int & c) const { node(M->nodes.at(i), mn, mx, f, c); }
    int enter(int slot, P3 p, P3 & pl) {
        const int inst = s.tlas_idx.at(slot);
        CHECK(object_visible(inst), "the walk entered hidden instance %d", inst);
        pl = rtxnp::xform_pos(s.inst[inst].world_inv, p); M = &s.meshes[s.inst[inst].blas_id];
        return inst;
    }
    int enter(int slot, P3 o, P3 d, P3 & co, P3 & cd) {
        const int inst = s.tlas_idx.at(slot);
        CHECK(object_visible(inst), "the walk entered hidden instance %d", inst);
        co = rtxnp::xform_pos(s.inst[inst].world_inv, o); cd = rtxnp::xform_dir(s.inst[inst].world_inv, d); M = &s.meshes[s.inst[inst].blas_id];
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
struct List {
    std::vector<float> t; std::vector<int32_t> o, s;
    explicit List(int K) : t(K > 0 ? K : 1), o(K > 0 ? K : 1), s(K > 0 ? K : 1) {}
    void get(int j, float & t_, int32_t & o_, int32_t & s_) const { t_ = t.at(j); o_ = o.at(j); s_ = s.at(j); }
    void set(int j, float t_, int32_t o_, int32_t s_) { t.at(j) = t_; o.at(j) = o_; s.at(j) = s_; }
};
struct Hit { float t; int32_t object, triangle; };

static int public_id(const Scene & s, int kind, int object) { return kind == rtxnp::KIND_TRI ? object : kind == rtxnp::KIND_SPHERE ? (int)s.inst.size() + object : (int)(s.inst.size() + s.spheres.size()) + object; }
static double len(const float v[3]) { return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }
static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static rtxnp::Answer nearest_exhaustive(const Scene & s, const Access & A, const float * row) {
    rtxnp::Answer a; a.kind = rtxnp::KIND_NONE; a.object = a.slot = -1; a.u = a.v = 0.0f; a.d2 = INFINITY;
    if (!rtxnp::row_is_live(row) || !A.row_visible()) return a;
    const P3 p = rtxnp::mk(row[0], row[1], row[2]);
    a.d2 = row[3] * row[3];
    for (size_t k = 0; k < s.spheres.size(); k++) if (A.sphere_visible((int)k)) rtxnp::offer(a, rtxnp::sphere_d2(p, rtxnp::ptr3(s.spheres[k].center), s.spheres[k].radius_squared), rtxnp::KIND_SPHERE, (int)k, -1, 0, 0);
    for (size_t k = 0; k < s.planes.size(); k++) if (A.plane_visible((int)k)) rtxnp::offer(a, rtxnp::plane_d2(p, rtxnp::ptr3(s.planes[k].normal), s.planes[k].distance), rtxnp::KIND_PLANE, (int)k, -1, 0, 0);
    for (size_t k = 0; k < s.inst.size(); k++) {
        if (!A.object_visible((int)k)) continue;
        const P3 pl = rtxnp::xform_pos(s.inst[k].world_inv, p);
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t t = 0; t < M.hot.size(); t++) {
            float u, v;
            rtxnp::offer(a, rtxnp::triangle_d2(rtxnp::sub(pl, rtxnp::ptr3(M.hot[t].position_0)), rtxnp::ptr3(M.hot[t].position_edge_1), rtxnp::ptr3(M.hot[t].position_edge_2), u, v), rtxnp::KIND_TRI, (int)k, (int)t, u, v);
        }
    }
    return a;
}
static std::vector<Hit> hits_exhaustive(const Scene & s, const Access & A, const float * row) {
    std::vector<Hit> all;
    if (!rtxhp::row_is_live(row) || !A.row_visible()) return all;
    const P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
    const float D = row[6];
    const int ic = (int)s.inst.size(), sn = (int)s.spheres.size();
    for (int i = 0; i < sn; i++) {
        if (!A.sphere_visible(i)) continue;
        float t0, t1;
        if (!rtxhp::sphere_roots(rtxnp::ptr3(s.spheres[i].center), s.spheres[i].radius_squared, o, d, t0, t1)) continue;
        if (rtxhp::in_range(t0, D)) all.push_back({ t0, ic + i, -1 });
        if (rtxhp::in_range(t1, D)) all.push_back({ t1, ic + i, -1 });
    }
    for (int i = 0; i < (int)s.planes.size(); i++) {
        if (!A.plane_visible(i)) continue;
        const float t = rtxhp::plane_t(rtxnp::ptr3(s.planes[i].normal), s.planes[i].distance, o, d);
        if (rtxhp::in_range(t, D)) all.push_back({ t, ic + sn + i, -1 });
    }
    for (int k = 0; k < ic; k++) {
        if (!A.object_visible(k)) continue;
        const P3 co = rtxnp::xform_pos(s.inst[k].world_inv, o), cd = rtxnp::xform_dir(s.inst[k].world_inv, d);
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t j = 0; j < M.hot.size(); j++) {
            float t, u, v;
            if (rtxhp::tri_test(rtxnp::ptr3(M.hot[j].position_0), rtxnp::ptr3(M.hot[j].position_edge_1), rtxnp::ptr3(M.hot[j].position_edge_2), co, cd, D, t, u, v)) all.push_back({ t, k, (int32_t)j });
        }
    }
    std::sort(all.begin(), all.end(), [](const Hit & a, const Hit & b) { return rtxhp::before(a.t, a.object, a.triangle, b.t, b.object, b.triangle); });
    return all;
}
static rtxsp::Answer sweep_exhaustive(const Scene & s, Access & A, const float * row) {
    rtxsp::Answer a; rtxsp::clear(a);
    if (!rtxsp::row_is_live(row) || !A.row_visible()) return a;
    const P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
    a.t = row[6];
    rtxsp::world_primitives(A, a, o, d, row[6], row[7]);
    for (size_t k = 0; k < s.inst.size(); k++) {
        if (!A.object_visible((int)k)) continue;
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

static double worst_ratio = 0.0;
static int worst_stack = 0;
static long rows_checked = 0, rows_answered = 0, rows_changed = 0, leaves_skipped = 0, hits_checked = 0;

static uint32_t pick_row_mask(int i) {
    const int k = i % 8;
    if (k == 0) return 0u;
    if (k < 4) return 1u << (rnd_u32() % 4);
    if (k < 6) { const uint32_t a = rnd_u32() % 4, b = (a + 1 + rnd_u32() % 3) % 4; return (1u << a) | (1u << b); }
    return 0xffffffffu;
}

// `rows` random rows of every kind against scene s under its masks; hide_all: the rows' masks share no bit with any object's
static void check_scene(const Scene & s, const char * what, int rows, float reach, bool hide_all) {
    int deepest = -1;
    for (const Mesh & m : s.meshes) if (m.inner_depth > deepest) deepest = m.inner_depth;
    const int need = rtxnp::stack_need(s.tlas_depth, deepest);
    CHECK(need <= RTX_MAX_STACK, "%s: the generator exceeded the stack bound (%d)", what, need);
    CHECK((int)s.masks.size() == s.objects(), "%s: one mask per object", what);
    Scene open = s;                                                         // the same scene with nothing hidden: what the filter changes
    for (uint32_t & m : open.masks) m = 0xffffffffu;
    for (int i = 0; i < rows; i++) {
        const uint32_t rm = hide_all ? 16u << (i % 4) : pick_row_mask(i);
        // ---- nearest
        {
            float row[4] = { rnd(-reach, reach), rnd(-reach, reach), rnd(-reach, reach), INFINITY };
            if (i % 5 == 1) row[3] = rnd(0.01f, reach);
            Access A{ s, rm }; Stack st(need > 0 ? need : 1);
            rtxnp::Answer w;
            rtxnp::walk(A, st, row, w);
            const rtxnp::Answer e = nearest_exhaustive(s, A, row);
            rows_checked++; leaves_skipped += A.hidden_skipped;
            if (st.high > worst_stack) worst_stack = st.high;
            CHECK(st.high <= need, "%s: stack %d above the stated %d", what, st.high, need);
            if (rm == 0u || hide_all) CHECK(w.kind == rtxnp::KIND_NONE && w.object == -1 && (rm != 0u || st.high == 0), "%s nearest row %d: a row that sees nothing got an answer", what, i);
            if (w.kind != rtxnp::KIND_NONE) { CHECK(A.object_visible(public_id(s, w.kind, w.object)), "%s nearest row %d: hidden object %d answers", what, i, public_id(s, w.kind, w.object)); rows_answered++; }
            { Access O{ open, 0xffffffffu }; Stack so(need > 0 ? need : 1); rtxnp::Answer u; rtxnp::walk(O, so, row, u); if (u.kind != w.kind || u.object != w.object || !same_bits(u.d2, w.d2)) rows_changed++; }
            if (e.kind == rtxnp::KIND_NONE) CHECK(w.kind == rtxnp::KIND_NONE && w.d2 == e.d2, "%s nearest row %d: an answer nothing visible justifies", what, i);
            else {
                const float dw = w.kind == rtxnp::KIND_NONE ? INFINITY : rtxnp::root(w.d2), de = rtxnp::root(e.d2);
                CHECK(dw >= de, "%s nearest row %d: walk %.9g below exhaustive %.9g", what, i, dw, de);
                if (e.kind != rtxnp::KIND_TRI) CHECK(w.kind == e.kind && w.object == e.object && w.d2 == e.d2, "%s nearest row %d: spheres and planes are never pruned", what, i);
                else {
                    const rtx_instance & I = s.inst[e.object];
                    const rtx_triangle_hot & t = s.meshes[I.blas_id].hot[e.slot];
                    const P3 p = rtxnp::mk(row[0], row[1], row[2]), pl = rtxnp::xform_pos(I.world_inv, p);
                    const float ap[3] = { pl.x - t.position_0[0], pl.y - t.position_0[1], pl.z - t.position_0[2] }, pw[3] = { p.x, p.y, p.z }, plv[3] = { pl.x, pl.y, pl.z };
                    const double S = len(ap) + len(t.position_edge_1) + len(t.position_edge_2);
                    float id[16]; identity(id);
                    const double W = memcmp(id, I.world_inv, 64) == 0 ? 0.0 : len(pw) + len(plv);
                    const double bound = rtxnp::distance_bound((float)S, (float)W);
                    const double excess = (w.kind == rtxnp::KIND_NONE ? (double)row[3] : (double)dw) - (double)de;
                    CHECK(excess <= bound, "%s nearest row %d: walk %.9g exceeds exhaustive %.9g by %.3g, bound %.3g", what, i, dw, de, excess, bound);
                    if (excess > 0 && excess / bound > worst_ratio) worst_ratio = excess / bound;
                }
            }
        }
        // ---- hits: K = 8 with a count, K = 3 without, count only
        {
            float row[7] = { rnd(-reach, reach), rnd(-reach, reach), rnd(-reach, reach), 0, 0, 0, INFINITY };
            for (int a = 0; a < 3; a++) row[3 + a] = rnd(-4.0f, 4.0f) - row[a];
            if (i % 5 == 2) row[6] = rnd(0.2f, 1.5f);
            Access E{ s, rm };
            const std::vector<Hit> all = hits_exhaustive(s, E, row);
            for (int form = 0; form < 3; form++) {
                const int K = form == 0 ? 8 : form == 1 ? 3 : 0;
                const bool counted = form != 1;
                Access A{ s, rm }; Stack st(need > 0 ? need : 1); List L(K);
                rtxhp::Tally w;
                rtxhp::walk(A, st, L, row, K, counted, w);
                rows_checked++;
                if (st.high > worst_stack) worst_stack = st.high;
                CHECK(st.high <= need, "%s: stack %d above the stated %d", what, st.high, need);
                CHECK(w.count <= (int)all.size(), "%s hits row %d form %d: count %d above the exhaustive %d", what, i, form, w.count, (int)all.size());
                if (rm == 0u || hide_all) CHECK(w.count == 0 && w.held == 0, "%s hits row %d: a row that sees nothing has hits", what, i);
                if (w.count > 0 && form == 0) rows_answered++;
                for (int j = 0; j < w.held; j++) {
                    CHECK(A.object_visible(L.o[j]), "%s hits row %d: hidden object %d is listed", what, i, L.o[j]);
                    CHECK(j == 0 || !rtxhp::before(L.t[j], L.o[j], L.s[j], L.t[j - 1], L.o[j - 1], L.s[j - 1]), "%s hits row %d: entries %d and %d out of order", what, i, j - 1, j);
                    bool known = false;
                    for (const Hit & h : all) if (same_bits(h.t, L.t[j]) && h.object == L.o[j] && h.triangle == L.s[j]) { known = true; break; }
                    CHECK(known, "%s hits row %d form %d: listed hit %d (t %.9g object %d slot %d) is no hit of the exhaustive search over the visible set", what, i, form, j, L.t[j], L.o[j], L.s[j]);
                    hits_checked++;
                }
            }
        }
        // ---- sweep
        {
            float row[8] = { rnd(-reach, reach), rnd(-reach, reach), rnd(-reach, reach), 0, 0, 0, INFINITY, 0 };
            const float speed = i % 3 == 0 ? 0.05f : i % 3 == 1 ? 1.0f : 7.0f;
            for (int a = 0; a < 3; a++) row[3 + a] = (rnd(-4.0f, 4.0f) - row[a]) * speed * 0.2f;
            row[7] = i % 4 == 0 ? rnd(0.5f, 1.5f) : i % 4 == 1 ? rnd(0.001f, 0.01f) : rnd(0.01f, 0.3f);
            if (i % 5 == 1) row[6] = rnd(0.01f, 2.0f) / speed;
            Access A{ s, rm }; Stack st(need > 0 ? need : 1);
            rtxsp::Answer w;
            rtxsp::walk(A, st, row, w);
            Access E{ s, rm };
            const rtxsp::Answer e = sweep_exhaustive(s, E, row);
            rows_checked++;
            if (st.high > worst_stack) worst_stack = st.high;
            CHECK(st.high <= need, "%s: stack %d above the stated %d", what, st.high, need);
            const float tw = w.kind == rtxnp::KIND_NONE ? INFINITY : w.t, te = e.kind == rtxnp::KIND_NONE ? INFINITY : e.t;
            CHECK(tw >= te, "%s sweep row %d: walk %.9g before exhaustive %.9g", what, i, tw, te);
            if (rm == 0u || hide_all) CHECK(w.kind == rtxnp::KIND_NONE && (rm != 0u || st.high == 0), "%s sweep row %d: a row that sees nothing got an answer", what, i);
            if (e.kind != rtxnp::KIND_TRI && e.kind != rtxnp::KIND_NONE) CHECK(w.kind == e.kind && w.object == e.object && w.t == e.t, "%s sweep row %d: spheres and planes are never pruned", what, i);
            if (w.kind != rtxnp::KIND_NONE) {
                CHECK(A.object_visible(public_id(s, w.kind, w.object)), "%s sweep row %d: hidden object %d stops the ball", what, i, public_id(s, w.kind, w.object));
                CHECK(w.t >= 0.0f && w.t < row[6], "%s sweep row %d: t %.9g outside [0, D)", what, i, w.t);
                rows_answered++;
            }
            if (s.inst.size() == 1 && s.inst[0].world[3] == 0.0f) CHECK(tw == te && w.kind == e.kind && w.object == e.object, "%s sweep row %d: one unmoved instance: walk %.9g is not the exhaustive %.9g", what, i, tw, te);
        }
    }
}

static void random_masks(Scene & s) { s.masks.clear(); for (int k = 0; k < s.objects(); k++) s.masks.push_back(rnd_u32() % 16u); }

int main() {
    const float zero[3] = { 0, 0, 0 };
    // one unmoved instance, chains and combs up to the stack bound (63 leaves of one slot = inner depth 61, need 62), and a balanced tree
    for (int shape = CHAIN; shape <= BALANCED; shape++)
        for (int leaf = 1; leaf <= 4; leaf += 3) {
            Scene s;
            const int n = shape == BALANCED ? 200 : 63 * leaf - (leaf > 1 ? 1 : 0);
            s.meshes.push_back(make_mesh(n, shape, leaf));
            s.inst.push_back(make_instance(0, 0.0f, zero));
            make_tlas(s, BALANCED, 1);
            s.masks.assign(1, 5u);                                          // seen by bits 0 and 2
            char what[64]; snprintf(what, sizeof what, "shape %d leaf %d", shape, leaf);
            check_scene(s, what, 160, 7.0f, false);
        }
    {   // deep TLAS over deep BLAS at the bound exactly (31 + 33 = 64), random masks: hidden instances all along the chain
        Scene s;
        s.meshes.push_back(make_mesh(34, CHAIN, 1));
        s.meshes.push_back(make_mesh(40, COMB, 2));
        for (int k = 0; k < 32; k++) { const float t[3] = { rnd(-8, 8), rnd(-8, 8), rnd(-8, 8) }; s.inst.push_back(make_instance(k % 3 == 2 ? 1 : 0, k % 2 ? rnd(-3, 3) : 0.0f, t)); }
        make_tlas(s, CHAIN, 1);
        CHECK(rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth) == RTX_MAX_STACK, "the deep scene sits at the bound (%d)", rtxnp::stack_need(s.tlas_depth, s.meshes[0].inner_depth));
        random_masks(s);
        check_scene(s, "deep TLAS over deep BLAS", 400, 14.0f, false);
        for (uint32_t & m : s.masks) m &= 15u;
        check_scene(s, "deep TLAS over deep BLAS, everything hidden", 60, 14.0f, true);
    }
    {   // coincident instances with different masks, spheres and planes, TLAS leaves of up to three instances some of which are hidden as a whole
        Scene s;
        s.meshes.push_back(make_mesh(120, BALANCED, 3));
        const float t0[3] = { 1.5f, -0.5f, 0.25f }, t1[3] = { -3.0f, 2.0f, 1.0f }, t2[3] = { 4.0f, 4.0f, -2.0f };
        s.inst.push_back(make_instance(0, 0.7f, t0)); s.inst.push_back(make_instance(0, 0.7f, t0));      // the same mesh twice in one place: masks 1 and 2
        s.inst.push_back(make_instance(0, 0.0f, t1)); s.inst.push_back(make_instance(0, 0.0f, t1));      // and again: masks 4 and 8
        s.inst.push_back(make_instance(0, -1.1f, zero));
        for (int k = 0; k < 6; k++) s.inst.push_back(make_instance(0, 0.3f * k, t2));                    // six in one place: two TLAS leaves, all of mask 8
        make_tlas(s, COMB, 3);
        rtx_sphere sp; memset(&sp, 0, sizeof sp); sp.center[0] = 2; sp.center[1] = 3; sp.center[2] = -1; sp.radius_squared = 2.25f; sp.radius_inv = 1.0f / 1.5f;
        s.spheres.push_back(sp); s.spheres.push_back(sp);
        rtx_plane pl; memset(&pl, 0, sizeof pl); pl.normal[1] = 1.0f; pl.distance = 7.0f; pl.u_axis[0] = 1.0f; pl.v_axis[2] = 1.0f;
        s.planes.push_back(pl);
        const uint32_t masks[] = { 1, 2, 4, 8, 15, 8, 8, 8, 8, 8, 8, /* spheres */ 3, 12, /* plane */ 6 };
        s.masks.assign(masks, masks + sizeof masks / sizeof masks[0]);
        check_scene(s, "coincident instances, hidden leaves, spheres, planes", 900, 9.0f, false);
        // the coincident pair: the row's mask chooses which of the two answers, at the same distance
        int pair_rows = 0;
        for (int i = 0; i < 400; i++) {
            const float row[4] = { t0[0] + rnd(-3, 3), t0[1] + rnd(-3, 3), t0[2] + rnd(-3, 3), INFINITY };
            rtxnp::Answer a[2];
            for (int k = 0; k < 2; k++) { Access A{ s, 1u << k }; Stack st(RTX_MAX_STACK); rtxnp::walk(A, st, row, a[k]); }
            CHECK(a[0].kind == a[1].kind && same_bits(a[0].d2, a[1].d2) && a[0].slot == a[1].slot, "coincident row %d: d2 %.9g and %.9g, slots %d and %d", i, a[0].d2, a[1].d2, a[0].slot, a[1].slot);
            if (a[0].kind != rtxnp::KIND_TRI) { CHECK(a[0].object == a[1].object, "coincident row %d: sphere or plane %d and %d", i, a[0].object, a[1].object); continue; }
            CHECK(a[0].object != 1 && a[1].object != 0, "coincident row %d: a hidden twin answers", i);
            if (a[0].object == 0) { CHECK(a[1].object == 1, "coincident row %d: mask 1 sees instance 0, mask 2 sees instance %d", i, a[1].object); pair_rows++; }
            else CHECK(a[0].object == a[1].object, "coincident row %d: objects %d and %d", i, a[0].object, a[1].object);
        }
        CHECK(pair_rows > 50, "rows whose nearest surface is the coincident pair (%d)", pair_rows);
        for (uint32_t & m : s.masks) m = 0u;
        check_scene(s, "a table that hides everything", 60, 9.0f, false);
        CHECK(rows_answered > 0, "rows were answered before the table hid everything");
    }
    printf("mask_check: %ld rows, %ld answered, %ld nearest rows the filter changed, %ld hidden instances passed over, %ld listed hits, deepest stack %d of %d, worst excess / bound %.4f\n",
           rows_checked, rows_answered, rows_changed, leaves_skipped, hits_checked, worst_stack, RTX_MAX_STACK, worst_ratio);
    CHECK(rows_answered > rows_checked / 8 && rows_changed > 100 && leaves_skipped > 1000 && hits_checked > 1000, "too little happened for the check to mean anything");
    if (fails) { printf("mask_check: %d FAILED\n", fails); return 1; }
    printf("mask_check: ok\n");
    return 0;
}
