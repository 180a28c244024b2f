// capsule_check.cpp — the walk and the tests of rtx_query_overlap_capsule (rtx_capsule_math.h) against the exhaustive search over the same
// functions, on generated trees, under the host sanitizers (make capsule_check).  No GPU, no ROCm.  The generator and the checks are
// overlap_check.cpp's, over capsule rows.
//   trees      chains, combs, left-deep chains and balanced trees for the BLAS and the TLAS, up to 62 of the RTX_MAX_STACK entries and to the
//              bound itself; TLAS leaves of 1 .. 3; duplicated slots; degenerate and NaN triangles; coincident instances, also with different
//              masks; TLAS leaves whose instances are all hidden from a row
//   rows       random capsules, capsules that contain everything, zero-length axes (balls), zero radii (segments), both (points), axes
//              along a coordinate axis (zero components of d), long thin capsules, hostile rows (NaN, inf, a negative radius)
//   checked    PROMISED of the header in all three forms: every listed overlap an overlap of the exhaustive search, in order, the K smallest
//              of what the walk found; count <= the exhaustive count (and equal but for rows within rounding of touching, which are counted);
//              any == (count > 0); the objects form == the distinct objects of the triangles form; no hidden object in any answer; a row of
//              mask 0 and a hostile row unanswered and not walked; the stack never above rtxnp::stack_need; every instance in exactly one
//              TLAS leaf; a ball's triangle test equals triangle_d2 <= r * r; a NaN slot never overlaps
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <set>
#include <utility>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_capsule_math.h"

using rtxnp::P3;

static uint32_t rng_state = 13579u;
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
    const Scene & s; uint32_t row_mask; const Mesh * M = nullptr; mutable long hidden_skipped = 0; long entered = 0;
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
    int enter(int slot, rtxcp::Frame & F) {
        const int inst = s.tlas_idx.at(slot);
        CHECK(object_visible(inst), "the walk entered hidden instance %d", inst);
        F = rtxcp::local_frame(F, s.inst[inst].world_inv); M = &s.meshes[s.inst[inst].blas_id];
        entered++;
        return inst;
    }
    void triangle(int i, P3 & p0, P3 & e1, P3 & e2) const { const rtx_triangle_hot & t = M->hot.at(i); p0 = rtxnp::ptr3(t.position_0); e1 = rtxnp::ptr3(t.position_edge_1); e2 = rtxnp::ptr3(t.position_edge_2); }
};
struct Stack {
    std::vector<int> node; int high = 0;
    explicit Stack(int cap) : node(cap) {}
    void push(int sp, int n) { node.at(sp) = n; if (sp + 1 > high) high = sp + 1; }      // at(): beyond the stated count is a failure
    void pop(int sp, int & n) const { n = node.at(sp); }
};
struct List {
    std::vector<int32_t> o, s;
    explicit List(int K) : o(K > 0 ? K : 1), s(K > 0 ? K : 1) {}
    void get(int j, int32_t & o_, int32_t & s_) const { o_ = o.at(j); s_ = s.at(j); }
    void set(int j, int32_t o_, int32_t s_) { o.at(j) = o_; s.at(j) = s_; }
};
typedef std::pair<int32_t, int32_t> Pair;

// every overlap of the visible set, by the header's functions, in ORDER
static std::vector<Pair> exhaustive(const Scene & s, const Access & A, const float * row) {
    std::vector<Pair> all;
    if (!rtxcp::row_is_live(row) || !A.row_visible()) return all;
    const rtxcp::Frame W = rtxcp::world_frame(row);
    const int ic = (int)s.inst.size(), sn = (int)s.spheres.size();
    for (int i = 0; i < sn; i++) if (A.sphere_visible(i) && rtxcp::sphere_overlaps(W, rtxnp::ptr3(s.spheres[i].center), s.spheres[i].radius_squared)) all.push_back(Pair(ic + i, -1));
    for (int i = 0; i < (int)s.planes.size(); i++) if (A.plane_visible(i) && rtxcp::plane_overlaps(W, rtxnp::ptr3(s.planes[i].normal), s.planes[i].distance)) all.push_back(Pair(ic + sn + i, -1));
    for (int k = 0; k < ic; k++) {
        if (!A.object_visible(k)) continue;
        const rtxcp::Frame F = rtxcp::local_frame(W, s.inst[k].world_inv);
        const Mesh & M = s.meshes[s.inst[k].blas_id];
        for (size_t j = 0; j < M.hot.size(); j++)
            if (rtxcp::triangle_overlaps(F, rtxnp::ptr3(M.hot[j].position_0), rtxnp::ptr3(M.hot[j].position_edge_1), rtxnp::ptr3(M.hot[j].position_edge_2))) all.push_back(Pair(k, (int32_t)j));
    }
    std::sort(all.begin(), all.end());
    return all;
}

static int worst_stack = 0;
static long rows_checked = 0, rows_answered = 0, rows_full = 0, rows_short = 0, leaves_skipped = 0, listed = 0, nan_slots_listed = 0;

static uint32_t pick_row_mask(int i) {
    const int k = i % 8;
    if (k == 0) return 0u;
    if (k < 3) return 1u << (rnd_u32() % 4);
    if (k < 5) { const uint32_t a = rnd_u32() % 4, b = (a + 1 + rnd_u32() % 3) % 4; return (1u << a) | (1u << b); }
    return 0xffffffffu;
}
// row kinds: 0 random capsule, 1 contains everything, 2 zero parts (ball / segment / point), 3 axis along a coordinate axis, 4 long and thin, 5 hostile
static void make_row(float * r, int kind, int i, float reach) {
    for (int a = 0; a < 3; a++) { r[a] = rnd(-reach, reach); r[3 + a] = rnd(-1.5f, 1.5f); }
    r[6] = rnd(0.02f, 0.8f);
    if (kind == 1) { for (int a = 0; a < 3; a++) r[a] = rnd(-1.0f, 1.0f); r[6] = 64.0f; }
    if (kind == 2) { const int z = 1 + i % 3; if (z & 1) r[3] = r[4] = r[5] = 0.0f; if (z & 2) r[6] = 0.0f; }
    if (kind == 3) { const int keep = i % 3; for (int a = 0; a < 3; a++) if (a != keep) r[3 + a] = (i & 4) ? -0.0f : 0.0f; }
    if (kind == 4) { for (int a = 0; a < 3; a++) r[3 + a] *= 8.0f; r[6] = (i & 1) ? 1e-3f : 0.0f; }
    if (kind == 5) {
        switch (i % 4) {
            case 0: r[i % 7] = NAN; break;
            case 1: r[(i / 4) % 7] = (i & 2) ? INFINITY : -INFINITY; break;
            case 2: r[6] = -0.25f; break;
            default: r[6] = -1e-30f; break;
        }
    }
}

template <int FORM> static void run_walk(const Scene & s, uint32_t rm, const float * row, int K, int need, List & L, rtxop::Tally & w, long & hidden, long & entered) {
    Access A{ s, rm }; Stack st(need > 0 ? need : 1);
    rtxcp::walk<FORM>(A, st, L, row, K, w);
    if (st.high > worst_stack) worst_stack = st.high;
    CHECK(st.high <= need, "stack %d above the stated %d", st.high, need);
    hidden = A.hidden_skipped; entered = A.entered;
}

// `rows` rows of every kind against scene s under its masks; hide_all: the rows' masks share no bit with any object's
static void check_scene(const Scene & s, const char * what, int rows, float reach, bool hide_all) {
    int deepest = -1;
    for (const Mesh & m : s.meshes) if (m.inner_depth > deepest) deepest = m.inner_depth;
    const int need = rtxnp::stack_need(s.tlas_depth, deepest);
    CHECK(need <= RTX_MAX_STACK, "%s: the generator exceeded the stack bound (%d)", what, need);
    CHECK((int)s.masks.size() == s.objects(), "%s: one mask per object", what);
    for (int i = 0; i < rows; i++) {
        const uint32_t rm = hide_all ? 16u << (i % 4) : pick_row_mask(i);
        const int kind = i % 16 == 15 ? 5 : i % 16 == 14 ? 1 : (i % 16) % 5 == 4 ? 4 : (i % 16) % 5;
        float row[7];
        make_row(row, kind == 1 && i % 32 == 30 ? 3 : kind, i, reach);
        const bool live = rtxcp::row_is_live(row);
        CHECK(live == (kind != 5), "%s row %d kind %d: liveness %d", what, i, kind, (int)live);
        Access E{ s, rm };
        const std::vector<Pair> all = exhaustive(s, E, row);
        std::set<int32_t> all_objects;
        for (const Pair & p : all) all_objects.insert(p.first);
        rows_checked++;
        if (!all.empty()) rows_answered++;
        long hidden = 0, entered = 0;
        // ---- TRIANGLES: K = 8, K = 3, count only
        std::set<Pair> found8;
        int count_tri = 0;
        for (int form = 0; form < 3; form++) {
            const int K = form == 0 ? 8 : form == 1 ? 3 : 0;
            List L(K); rtxop::Tally w;
            run_walk<rtxop::FORM_TRIANGLES>(s, rm, row, K, need, L, w, hidden, entered);
            if (form == 0) { leaves_skipped += hidden; count_tri = w.count; }
            CHECK(w.count == count_tri, "%s row %d: the count depends on K (%d, %d)", what, i, w.count, count_tri);
            CHECK(w.count <= (int)all.size(), "%s row %d form %d: count %d above the exhaustive %d", what, i, form, w.count, (int)all.size());
            CHECK(w.held == (w.count < K ? w.count : K), "%s row %d form %d: %d entries held of count %d", what, i, form, w.held, w.count);
            if (!live || rm == 0u || hide_all) CHECK(w.count == 0 && w.held == 0 && entered == 0, "%s row %d: a row that sees nothing has overlaps or was walked", what, i);
            for (int j = 0; j < w.held; j++) {
                CHECK(E.object_visible(L.o[j]), "%s row %d: hidden object %d is listed", what, i, L.o[j]);
                CHECK(j == 0 || rtxop::before(L.o[j - 1], L.s[j - 1], L.o[j], L.s[j]), "%s row %d: entries %d and %d out of order or equal", what, i, j - 1, j);
                CHECK(std::binary_search(all.begin(), all.end(), Pair(L.o[j], L.s[j])), "%s row %d form %d: listed overlap %d (object %d slot %d) is none of the exhaustive search", what, i, form, j, L.o[j], L.s[j]);
                if (form == 0) found8.insert(Pair(L.o[j], L.s[j]));
                listed++;
            }
            if (form == 0 && w.count == (int)all.size()) {                      // everything found: the list is the exhaustive list's first K
                rows_full++;
                for (int j = 0; j < w.held; j++) CHECK(all[j] == Pair(L.o[j], L.s[j]), "%s row %d: entry %d is not the exhaustive list's", what, i, j);
            } else if (form == 0) rows_short++;
            if (form == 1) { int j = 0; for (const Pair & p : found8) { if (j >= w.held) break; CHECK(p == Pair(L.o[j], L.s[j]), "%s row %d: K = 3 is no prefix of K = 8 at %d", what, i, j); j++; } }
        }
        // ---- OBJECTS: K = 8 and count only; the distinct objects of the triangles form when that found everything
        {
            List L(8); rtxop::Tally w, w0; List L0(0);
            run_walk<rtxop::FORM_OBJECTS>(s, rm, row, 8, need, L, w, hidden, entered);
            run_walk<rtxop::FORM_OBJECTS>(s, rm, row, 0, need, L0, w0, hidden, entered);
            CHECK(w.count == w0.count, "%s row %d: the objects count depends on K", what, i);
            CHECK(w.count <= (int)all_objects.size(), "%s row %d: %d objects above the exhaustive %d", what, i, w.count, (int)all_objects.size());
            if (count_tri == (int)all.size()) CHECK(w.count == (int)all_objects.size(), "%s row %d: %d objects, the triangles form names %d", what, i, w.count, (int)all_objects.size());
            for (int j = 0; j < w.held; j++) {
                CHECK(L.s[j] == -1 && all_objects.count(L.o[j]) == 1, "%s row %d: listed object %d (slot %d) is none", what, i, L.o[j], L.s[j]);
                CHECK(j == 0 || L.o[j - 1] < L.o[j], "%s row %d: objects %d and %d repeated or out of order", what, i, L.o[j - 1], L.o[j]);
            }
            if (w.count == (int)all_objects.size()) { int j = 0; for (int32_t o : all_objects) { if (j >= w.held) break; CHECK(o == L.o[j], "%s row %d: object entry %d", what, i, j); j++; } }
        }
        // ---- ANY
        {
            List L0(0); rtxop::Tally w;
            run_walk<rtxop::FORM_ANY>(s, rm, row, 0, need, L0, w, hidden, entered);
            CHECK(w.count == (count_tri > 0 ? 1 : 0), "%s row %d: any %d, count %d", what, i, w.count, count_tri);
        }
        // a NaN slot is never an overlap
        for (const Pair & p : all) if (p.second >= 0) {
            const rtx_triangle_hot & t = s.meshes[s.inst[p.first].blas_id].hot[p.second];
            bool nan = false;
            for (int a = 0; a < 3; a++) nan = nan || t.position_0[a] != t.position_0[a] || t.position_edge_1[a] != t.position_edge_1[a] || t.position_edge_2[a] != t.position_edge_2[a];
            if (nan) nan_slots_listed++;
        }
    }
}

static void random_masks(Scene & s) { s.masks.clear(); for (int k = 0; k < s.objects(); k++) s.masks.push_back(rnd_u32() % 16u); }

int main() {
    const float zero[3] = { 0, 0, 0 };
    // one unmoved instance, chains and combs up to the stack bound (63 leaves of one slot = inner depth 61, need 62), and a balanced tree
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
    {   // deep TLAS over deep BLAS at the bound exactly (31 + 33 = 64), random masks: hidden instances all along the chain
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
    {   // coincident instances with different masks, spheres and planes, TLAS leaves of up to three instances some of which are hidden as a whole
        Scene s;
        s.meshes.push_back(make_mesh(120, BALANCED, 3, true));
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
        check_scene(s, "coincident instances, hidden leaves, spheres, planes", 1280, 8.0f, false);
        // the coincident pair: the row's mask chooses which of the two is listed, with the same slots
        int pair_rows = 0;
        for (int i = 0; i < 300; i++) {
            float row[7];
            make_row(row, 0, i, 2.0f);
            for (int a = 0; a < 3; a++) row[a] += t0[a];
            List L[2] = { List(8), List(8) }; rtxop::Tally w[2];
            long h, e;
            for (int k = 0; k < 2; k++) run_walk<rtxop::FORM_TRIANGLES>(s, 1u << k, row, 8, RTX_MAX_STACK, L[k], w[k], h, e);
            int n0 = 0, n1 = 0;
            for (int j = 0; j < w[0].held; j++) { CHECK(L[0].o[j] != 1, "coincident row %d: the hidden twin is listed", i); if (L[0].o[j] == 0) n0++; }
            for (int j = 0; j < w[1].held; j++) { CHECK(L[1].o[j] != 0, "coincident row %d: the hidden twin is listed", i); if (L[1].o[j] == 1) n1++; }
            if (w[0].count <= 8 && w[1].count <= 8) {
                CHECK(n0 == n1, "coincident row %d: %d slots of instance 0, %d of its twin", i, n0, n1);
                int a = 0, b = 0;
                while (a < w[0].held && b < w[1].held) {
                    while (a < w[0].held && L[0].o[a] != 0) a++;
                    while (b < w[1].held && L[1].o[b] != 1) b++;
                    if (a < w[0].held && b < w[1].held) { CHECK(L[0].s[a] == L[1].s[b], "coincident row %d: slots %d and %d", i, L[0].s[a], L[1].s[b]); a++; b++; }
                }
                if (n0 > 0) pair_rows++;
            }
        }
        CHECK(pair_rows > 30, "rows that overlap the coincident pair (%d)", pair_rows);
        for (uint32_t & m : s.masks) m = 0u;
        check_scene(s, "a table that hides everything", 64, 8.0f, false);
    }
    {   // a ball's triangle test is triangle_d2 <= r * r behind the guard and the bounds; a segment through a face's interior pierces at r == 0
        int agree = 0, pierced = 0;
        for (int i = 0; i < 20000; i++) {
            const P3 p0 = rtxnp::mk(rnd(-2, 2), rnd(-2, 2), rnd(-2, 2)), e1 = rtxnp::mk(rnd(-1, 1), rnd(-1, 1), rnd(-1, 1)), e2 = rtxnp::mk(rnd(-1, 1), rnd(-1, 1), rnd(-1, 1));
            rtxcp::Frame F; F.p = rtxnp::mk(rnd(-2, 2), rnd(-2, 2), rnd(-2, 2)); F.d = rtxnp::mk(0.0f, 0.0f, 0.0f); F.r = rnd(0.0f, 1.5f);
            float u, v;
            const bool want = rtxnp::triangle_d2(rtxnp::sub(F.p, p0), e1, e2, u, v) <= F.r * F.r;
            CHECK(rtxcp::triangle_overlaps(F, p0, e1, e2) == want, "ball %d: the triangle test is not triangle_d2 <= r * r", i);
            agree += want;
            const float a = rnd(0.2f, 0.6f), b = rnd(0.1f, 0.3f);
            const P3 q = rtxnp::add(p0, rtxnp::add(rtxnp::scale(e1, a), rtxnp::scale(e2, b))), n = rtxop::cross(e1, e2);
            F.p = rtxnp::sub(q, n); F.d = rtxnp::scale(n, 2.0f); F.r = 0.0f;
            if (rtxnp::dot(n, n) > 1e-2f) { CHECK(rtxcp::triangle_overlaps(F, p0, e1, e2), "segment %d through a face's interior does not pierce", i); pierced++; }
            F.d = rtxnp::scale(n, 0.5f);                                       // stops short of the plane, |n| / 2 away
            if (rtxnp::dot(n, n) > 1e-2f) CHECK(!rtxcp::triangle_overlaps(F, p0, e1, e2), "segment %d that stops short of the plane overlaps", i);
        }
        CHECK(agree > 1000 && pierced > 10000, "too few ball overlaps (%d) or pierced faces (%d)", agree, pierced);
    }
    printf("capsule_check: %ld rows, %ld with an overlap, %ld where the walk found every overlap, %ld short of the exhaustive count, %ld hidden instances passed over, %ld listed overlaps, deepest stack %d of %d\n",
           rows_checked, rows_answered, rows_full, rows_short, leaves_skipped, listed, worst_stack, RTX_MAX_STACK);
    CHECK(nan_slots_listed == 0, "%ld NaN slots overlap", nan_slots_listed);
    CHECK(rows_short * 500 <= rows_checked, "the walk misses overlaps of the exhaustive search on %ld of %ld rows: NODE is not conservative", rows_short, rows_checked);
    CHECK(rows_answered > rows_checked / 8 && leaves_skipped > 1000 && listed > 5000 && worst_stack >= 62, "too little happened for the check to mean anything");
    if (fails) { printf("capsule_check: %d FAILED\n", fails); return 1; }
    printf("capsule_check: ok\n");
    return 0;
}
