// rtx_hits_math.h — the arithmetic AND the walk of all-hits segment queries (include/rtx.h: rtx_query_hits), written once and compiled twice
// like rtx_nearest_math.h: by hipcc into k_query_hits (rtx_hits.h) and by the host compiler into rtxh_query_hits / rtxh_query_hits_exhaustive
// (host/rtx_host.cpp) and hits_check.cpp.  Unfused fp32 (-ffp-contract=off), correctly rounded '/' and sqrtf on both sides, every sum of three
// products in vdot's order x + (y + z); min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b (a NaN gives b).  So every function here
// returns the same bits on the CPU and on gfx950.  Plain C++: no HIP types.  This comment is the specification.
//
// ROW      (ox, oy, oz, dx, dy, dz, D): the rows of rtx_query_occluded.  A row is LIVE when the direction is not (+-0, +-0, +-0), all six
//          components are finite and D > 0 (a NaN D is not; +INFINITY is).  A dead row has count 0, an empty list, and is not walked.
// HIT      anything the reference's own tests accept against D, spelled as rtx_trace.h spells them.  EPS = RAY_EPSILON = 0.005.
//   triangle  tri_test with tmax = D in the instance's local ray: co = xform_pos(world_inv, o), cd = xform_dir(world_inv, d), as k_trace derives
//             them (the inverse direction of the box tests is 1 / cd per component).  h = cd x e2, a = e1.h, f = 1 / a, s = co - p0,
//             u = f * (s.h), qq = s x e1, v = f * (cd.qq), t = f * (e2.qq); a hit iff 0 < u < 1, 0 < v, u + v < 1 and EPS < t < D.  t is in
//             units of |d| (cd is not normalised), so it is comparable across instances and with spheres and planes.
//   plane     plane_t: t = -(n.o + distance) / (n.d), a hit iff EPS < t < D.
//   sphere    sphere_closest's arithmetic: oc = o - c, a = d.d, b = 2 * (oc.d), c = oc.oc - radius_squared, disc = b*b - 4*a*c, a candidate
//             pair iff disc >= 0: k = -(1 / (2*a)), t0 = (b + sqrtf(disc)) * k, t1 = (b - sqrtf(disc)) * k; EACH of t0, t1 is a hit iff
//             EPS < t < D.  A ray through a sphere crosses it twice, so crossing parity stays meaningful; a tangent (disc == 0) yields two
//             equal hits.  (rtx_query_occluded uses Sphere::intersect's other arithmetic: the two calls may differ on spheres.)
//   Every comparison is strict; a NaN never hits.
// ORDER    hits are ordered by (t, object_id, triangle_id) ascending, ids in the public numberings of rtx_query_closest (instances, then
//          spheres, then planes; triangle_id = the triangle's slot in its BLAS, -1 for spheres and planes).  The list is the first K of them:
//          it does not depend on the order of the walk or on the tree, only on WHICH hits the walk finds.  A BLAS whose leaves share
//          triangles (the spatial splits of the reference's SBVH) holds such a triangle once per slot, and every slot is a hit of its own.
// WALK     (walk() below)
//   1. Spheres ascending (t0 then t1), planes ascending, then the TLAS from its root; the list and the count take every hit (offer()).
//   2. bound = D.  The one exception: when no count is requested and the list holds K hits, bound = the t of the K-th (the list's last).
//   3. A node is entered iff slab_test(box, origin, inverse direction, bound) — AABB::intersect in the reference form, on every node, roots
//      included:  t0 = (min - o) * inv, t1 = (max - o) * inv per axis, t_near = max(max(EPS, tmin.x), max(tmin.y, tmin.z)),
//      t_far = min(min(bound, tmax.x), min(tmax.y, tmax.z)), pass iff t_near < t_far.  No NaN-free fast path, no plane-membership search.
//   4. Of an inner node's two children the one with the smaller t_near goes first, the left one when tl <= tr (or when only it passes).
//   5. The other child, if it passes, is pushed with its key and tested AGAIN against the then-current bound when popped.  key = -inf when
//      tmax.x is NaN, else t_near: for a node that passed once, slab_test against a later, smaller bound is exactly key < bound
//      (slab_test_key, rtx_trace.h), so the re-test reads no memory.
//   6. A TLAS leaf takes its instances in tlas_indices order, stepped through in two registers, not on the stack; a BLAS leaf its slots in order.
//   7. The triangle test always uses tmax = D: only boxes see the shrunken bound.  A hit at or beyond the K-th of a full list changes nothing.
//   FILTER (rtx_query_hits_filtered): the rule and the places of rtx_nearest_math.h's FILTER — a row whose mask is 0 has count 0 and an empty
//   list without a walk, a hidden sphere or plane is passed over in step 1, a hidden instance in step 6 before its matrix or its BLAS is
//   touched.  Hidden objects are neither listed nor counted; PROMISED holds against the exhaustive search over the visible primitives.
//   With a count the bound never moves and the walk visits exactly the nodes a segment of length D passes: the node set of the reference's
//   any-hit walk had it not stopped at its first hit.  STACK: a push happens only at an inner node and leaves one sibling per level of the
//   current path: at most rtxnp::stack_need() entries, by the argument of rtx_nearest_math.h.  The caller checks it; there is no overflow path.
// OUTPUTS  of hit (t, object, triangle): what rtx_query_closest reports had that hit been the closest — the accept branches rebuild_triangle_hit,
//          rebuild_sphere_hit, rebuild_plane_hit (rtx_shade.h) with zero differentials.  u, v of a triangle are not kept during the walk: tri_test
//          runs again on the listed triangle (the same function: the same bits).
//            triangle  position = xform_pos(world, co + cd * t); normal, uv: rtxnp::triangle_outputs at (u, v)
//            sphere    position = o + d * t, normal = (position - c) * radius_inv, uv from the normal as rebuild_sphere_hit
//            plane     position = o + d * t, normal = n, uv = (position.u_axis, position.v_axis)
//          Entries j >= min(count, K) hold the miss values: distance +inf, position / normal / uv 0, ids -1.
// PROMISED   every listed hit is a hit of the exhaustive search (every primitive, no boxes, the same functions) with the same bits, and
//            count <= the exhaustive count; with a count, the list is the first K, in ORDER, of the hits the walk found.
// NOT PROMISED  equality with the exhaustive list on every row.  The reference's box test can reject a box whose triangle its triangle test
//            accepts — a flat box where t_near == t_far, a box plane within an ulp of the hit, a hit within an ulp of EPS or D — which is the
//            reference's behaviour and rtx_query_closest's.  Without a count a hit whose t EQUALS the K-th hit's may likewise stay unseen
//            behind a box (t_near < bound is strict), so lists with and without a count may differ on such rows.
// MARGIN   (margin() below) how far tri_test's u, v and t may lie from their exact values, for tests that compare with fp64.  u = 2^-24.
//          h and qq: two products and a difference per component, 3u |cd||e2| and 3u |s||e1|; a dot product adds 3u of its terms' sizes; f = 1 / a
//          and the final product one u each; s = co - p0 one u |s|.  With kappa = |cd||e1||e2| / |a| (1 / (sin of the edges' angle * cos of the
//          ray's angle to the normal): the conditioning of the system) that is under 16u * kappa * scale with
//            scale = 1 + |s| / min(|e1|, |e2|)          for u and for v (their sum: both margins and the sum's own rounding, 2 margins + u),
//            scale = (|s| + |e1| + |e2|) / |cd|         for t.
//          A transformed instance moves co by 4u W and cd likewise, W = |o| + |co| (xform_pos rounds four times): add 8 W / min(|e1|, |e2|)
//          resp. 8 W / |cd| to the scale.  An identity matrix is exact: W = 0.  margin(kappa, scale) = 16 * 2^-24 * kappa * scale.
// OUT OF SCOPE  hits beyond RTX_QUERY_MAX_HITS per row, an any-hit callback or per-material filtering (FILTER hides whole objects by mask, nothing finer), a per-ray tmin other than RAY_EPSILON,
//          signed distance as a single call, barycentrics as a channel, the rtx_group_* path.
#pragma once
#include <stdint.h>
#include "rtx_nearest_math.h"

namespace rtxhp {

using rtxnp::P3;
using rtxnp::mk;
using rtxnp::add;
using rtxnp::sub;
using rtxnp::scale;
using rtxnp::dot;
using rtxnp::ptr3;
using rtxnp::xform_pos;
using rtxnp::xform_dir;
using rtxnp::is_finite;
using rtxnp::infinity;

enum { MAX_HITS = 8 };                                         // RTX_QUERY_MAX_HITS
RTX_HDF float eps() { return 0.005f; }                         // RAY_EPSILON, rtx_trace.h
RTX_HDF float min_ref(float a, float b) { return a < b ? a : b; }
RTX_HDF float max_ref(float a, float b) { return a > b ? a : b; }
RTX_HDF P3 cross(P3 l, P3 r) { return mk(l.y * r.z - l.z * r.y, l.z * r.x - l.x * r.z, l.x * r.y - l.y * r.x); }
RTX_HDF P3 rcp(P3 a) { return mk(1.0f / a.x, 1.0f / a.y, 1.0f / a.z); }

RTX_HDF bool row_is_live(const float * r) {
    if ((r[3] == 0.0f) & (r[4] == 0.0f) & (r[5] == 0.0f)) return false;
    for (int k = 0; k < 6; k++) if (!is_finite(r[k])) return false;
    return r[6] > 0.0f;
}

// slab_test_key of rtx_trace.h: pass, and the key of the pop-time re-test; t_near orders the children
RTX_HDF bool slab_test(P3 mn, P3 mx, P3 o, P3 inv, float bound, float & t_near, float & key) {
    const P3 t0 = mk((mn.x - o.x) * inv.x, (mn.y - o.y) * inv.y, (mn.z - o.z) * inv.z);
    const P3 t1 = mk((mx.x - o.x) * inv.x, (mx.y - o.y) * inv.y, (mx.z - o.z) * inv.z);
    const P3 tmin = mk(min_ref(t0.x, t1.x), min_ref(t0.y, t1.y), min_ref(t0.z, t1.z));
    const P3 tmax = mk(max_ref(t0.x, t1.x), max_ref(t0.y, t1.y), max_ref(t0.z, t1.z));
    t_near = max_ref(max_ref(eps(), tmin.x), max_ref(tmin.y, tmin.z));
    const float t_far = min_ref(min_ref(bound, tmax.x), min_ref(tmax.y, tmax.z));
    key = (tmax.x != tmax.x) ? -infinity() : t_near;
    return t_near < t_far;
}

RTX_HDF bool tri_test(P3 p0, P3 edge_1, P3 edge_2, P3 co, P3 cd, float tmax, float & t, float & u, float & v) {
    const P3 h = cross(cd, edge_2);
    const float a = dot(edge_1, h);
    const float f = 1.0f / a;
    const P3 s = sub(co, p0);
    u = f * dot(s, h);
    if (!((u > 0.0f) & (u < 1.0f))) return false;
    const P3 qq = cross(s, edge_1);
    v = f * dot(cd, qq);
    if (!((v > 0.0f) & ((u + v) < 1.0f))) return false;
    t = f * dot(edge_2, qq);
    return (t > eps()) & (t < tmax);
}
RTX_HDF float plane_t(P3 n, float distance, P3 o, P3 d) { return -(dot(n, o) + distance) / dot(n, d); }
RTX_HDF bool sphere_roots(P3 center, float radius_squared, P3 o, P3 d, float & t0, float & t1) {
    const P3 oc = sub(o, center);
    const float a = dot(d, d);
    const float b = 2.0f * dot(oc, d);
    const float c = dot(oc, oc) - radius_squared;
    const float disc = b * b - 4.0f * a * c;
    if (!(disc >= 0.0f)) return false;
    const float sqrt_d = rtxnp::root(disc);
    const float inv_denom = -(1.0f / (2.0f * a));
    t0 = (b + sqrt_d) * inv_denom;
    t1 = (b - sqrt_d) * inv_denom;
    return true;
}
RTX_HDF bool in_range(float t, float D) { return (t > eps()) & (t < D); }

// ORDER: (t, object, triangle) ascending
RTX_HDF bool before(float t, int32_t object, int32_t triangle, float t2, int32_t object2, int32_t triangle2) {
    if (t < t2) return true;
    if (!(t == t2)) return false;
    if (object != object2) return object < object2;
    return triangle < triangle2;
}

RTX_HDF float margin(float kappa, float scale_) { return 16.0f * 5.9604644775390625e-08f * kappa * scale_; }

// the accept branches at a listed hit
RTX_HDF P3 point_at(P3 o, P3 d, float t) { return add(o, scale(d, t)); }
RTX_HDF void sphere_outputs(P3 o, P3 d, float t, P3 center, float radius_inv, P3 & point, P3 & normal, float & tu, float & tv) {
    const float ONE_OVER_PI = 0.31830988618f, ONE_OVER_TWO_PI = 0.15915494309f;
    point = point_at(o, d, t);
    normal = scale(sub(point, center), radius_inv);
    tu = rtx_atan2f(normal.z, normal.x) * ONE_OVER_TWO_PI + 0.5f;
    tv = rtx_acosf(normal.y) * ONE_OVER_PI + 0.5f;
}
RTX_HDF void plane_outputs(P3 o, P3 d, float t, P3 n, P3 u_axis, P3 v_axis, P3 & point, P3 & normal, float & tu, float & tv) {
    point = point_at(o, d, t);
    normal = n;
    tu = dot(point, u_axis); tv = dot(point, v_axis);
}

// what a row's walk keeps: the hits seen, the entries the list holds, the bound of the box tests
struct Tally { int32_t count, held; float bound; };

// One hit.  List gives get(j, t, object, triangle) and set(j, t, object, triangle) for entries 0 .. K - 1.  A sorted insert over at most K
// entries; the loop bound is K, the same for every lane.  K == 0: count only.
template <typename List>
RTX_HDF void offer(List & L, const int K, const bool shrink, Tally & w, const float t, const int32_t object, const int32_t triangle) {
    w.count++;
    if (K <= 0) return;
    int e = w.held;                                                        // the entry the hit starts at, before it moves forward
    if (w.held == K) {
        float lt; int32_t lo, ls;
        L.get(K - 1, lt, lo, ls);
        if (!before(t, object, triangle, lt, lo, ls)) return;
        e = K - 1;
    } else w.held++;
    bool placed = false;
    for (int j = K - 1; j > 0; j--) {
        if (!placed && j <= e) {
            float pt; int32_t po, ps;
            L.get(j - 1, pt, po, ps);
            if (before(t, object, triangle, pt, po, ps)) L.set(j, pt, po, ps);
            else { L.set(j, t, object, triangle); placed = true; }
        }
    }
    if (!placed) L.set(0, t, object, triangle);
    if (shrink && w.held == K) { float lt; int32_t lo, ls; L.get(K - 1, lt, lo, ls); w.bound = lt; }
}

// spheres and planes of a live row: step 1 of the walk, and of the exhaustive search
template <typename Scene, typename List>
RTX_HDF void world_primitives(Scene & sc, List & L, const int K, const bool shrink, Tally & w, const P3 o, const P3 d, const float D) {
    const int32_t ic = sc.instance_count(), sn = sc.sphere_count();
    for (int i = 0; i < sn; i++) {
        if (!sc.sphere_visible(i)) continue;
        P3 c; float r2, t0, t1;
        sc.sphere(i, c, r2);
        if (!sphere_roots(c, r2, o, d, t0, t1)) continue;
        if (in_range(t0, D)) offer(L, K, shrink, w, t0, ic + i, -1);
        if (in_range(t1, D)) offer(L, K, shrink, w, t1, ic + i, -1);
    }
    for (int i = 0; i < sc.plane_count(); i++) {
        if (!sc.plane_visible(i)) continue;
        P3 n; float dist;
        sc.plane(i, n, dist);
        const float t = plane_t(n, dist, o, d);
        if (in_range(t, D)) offer(L, K, shrink, w, t, ic + sn + i, -1);
    }
}

// The walk.  Scene gives the records as for rtxnp::walk, plus instance_count() and enter(slot, o, d, co, cd) (makes the BLAS of instance
// tlas_indices[slot] current, gives the local ray, returns that instance) and FILTER's predicates.  Stack gives push(sp, node, key) and pop(sp, node, key).
// counted: a count is requested, the bound stays D.
template <typename Scene, typename Stack, typename List>
RTX_HDF void walk(Scene & sc, Stack & st, List & L, const float * row, const int K, const bool counted, Tally & w) {
    w.count = 0; w.held = 0; w.bound = 0.0f;
    if (!row_is_live(row) || !sc.row_visible()) return;
    const P3 o = mk(row[0], row[1], row[2]), d = mk(row[3], row[4], row[5]);
    const float D = row[6];
    const bool shrink = !counted;
    w.bound = D;
    world_primitives(sc, L, K, shrink, w, o, d, D);
    if (sc.tlas_nodes() <= 0) return;
    const P3 winv = rcp(d);
    P3 co = o, cd = d, cinv = winv;
    int sp = 0, floor_sp = 0, cur = -1, first = 0, count = 0, tl_i = 0, tl_end = 0, inst = 0;
    bool in_blas = false;
    float tn, key;
    { P3 mn, mx; sc.tlas_node(0, mn, mx, first, count); if (slab_test(mn, mx, co, cinv, w.bound, tn, key)) cur = 0; }
    for (;;) {
        if (cur < 0) {
            if (in_blas && sp == floor_sp) { in_blas = false; co = o; cd = d; cinv = winv; }      // this instance is done: back to world space
            if (!in_blas && tl_i < tl_end) {                                                      // the next instance of the TLAS leaf
                if (!sc.instance_visible(tl_i)) { tl_i++; continue; }                             // FILTER: hidden from this row
                inst = sc.enter(tl_i++, o, d, co, cd);
                cinv = rcp(cd);
                P3 mn, mx; sc.blas_node(0, mn, mx, first, count);
                in_blas = true; floor_sp = sp;
                if (slab_test(mn, mx, co, cinv, w.bound, tn, key)) cur = 0;
                continue;
            }
            if (sp == 0) break;
            int node;
            sp--; st.pop(sp, node, key);
            if (!(key < w.bound)) continue;
            cur = node;
            P3 mn, mx;
            if (in_blas) sc.blas_node(cur, mn, mx, first, count); else sc.tlas_node(cur, mn, mx, first, count);
        }
        if ((count & 0x3fffffff) > 0) {                                                           // a leaf: (first, count) of node cur
            const int n = count & 0x3fffffff;
            if (in_blas) {
                for (int i = first; i < first + n; i++) {
                    P3 p0, e1, e2; float t, u, v;
                    sc.triangle(i, p0, e1, e2);
                    if (tri_test(p0, e1, e2, co, cd, D, t, u, v)) offer(L, K, shrink, w, t, inst, i);
                }
            } else { tl_i = first; tl_end = first + n; }
            cur = -1;
            continue;
        }
        P3 lmn, lmx, rmn, rmx; int lf, lc, rf, rc;
        const int left = first;
        if (in_blas) { sc.blas_node(left, lmn, lmx, lf, lc); sc.blas_node(left + 1, rmn, rmx, rf, rc); }
        else         { sc.tlas_node(left, lmn, lmx, lf, lc); sc.tlas_node(left + 1, rmn, rmx, rf, rc); }
        float tl, tr, kl, kr;
        const bool pl = slab_test(lmn, lmx, co, cinv, w.bound, tl, kl), pr = slab_test(rmn, rmx, co, cinv, w.bound, tr, kr);
        const bool left_first = pl && (!pr || tl <= tr);
        if (pl && pr) { st.push(sp, left_first ? left + 1 : left, left_first ? kr : kl); sp++; }
        if (pl || pr) { cur = left_first ? left : left + 1; first = left_first ? lf : rf; count = left_first ? lc : rc; }
        else cur = -1;
    }
}

}  // namespace rtxhp
