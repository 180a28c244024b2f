// rtx_overlap_math.h — the arithmetic AND the walk of box-overlap queries (include/rtx.h: rtx_query_overlap), written once and compiled twice
// like rtx_hits_math.h: by hipcc into k_query_overlap (rtx_overlap.h) and by the host compiler into rtxh_query_overlap /
// rtxh_query_overlap_exhaustive (host/rtx_host.cpp) and overlap_check.cpp.  Unfused fp32 (-ffp-contract=off), correctly rounded '/' and sqrtf
// on both sides, every sum of three products in vdot's order x + (y + z); min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b (a NaN
// gives b).  So every function here returns the same bits on the CPU and on gfx950.  Plain C++: no HIP types.  This comment is the
// specification.
//
// ROW      ten floats: centre c (3), half extents h (3), rotation quaternion q = (x, y, z, w), the convention of rtx_update_instances.  The
//          quaternion is normalised here, q / sqrtf(q.q) per component, and becomes a matrix by the spelling of rtxu::world_matrix
//          (rtx_update_math.h); the box axes a_0, a_1, a_2 are that matrix's columns (cells k, 4 + k, 8 + k).  A box posed like an instance
//          whose quaternion has sqrtf(q.q) == 1 therefore has that instance's axes bit for bit.  The box is the set c + sum x_k a_k with
//          |x_k| <= h_k.  A row is LIVE when all ten floats are finite, every half extent is >= 0 and q.q is finite and > 0.  Zero half extents
//          are allowed: a point, a segment and a rectangle are valid boxes.  A dead row overlaps nothing, has count 0 and an empty list, and is
//          not walked.
// FRAME    what the tests read: c, a_k, h, and E_j = g_0 |a_0.j| + (g_1 |a_1.j| + g_2 |a_2.j|) with g_k = h_k / (a_k . a_k), the box's own
//          AABB c +- E.  In an instance's local frame c_l = xform_pos(world_inv, c), a_k = xform_dir(world_inv, a_k), h unchanged, E from the
//          local axes.  Every test reads the box as the set |a_k . (p - c)| <= h_k: exact for a rigid pose, the only kind the host lets
//          through (the rigid rule of rtx_query_nearest: its 2^-12 admits a uniform scale of a part in 10^4, which scales the axes and so the box), and the division by a_k . a_k keeps E the AABB of
//          that same set, so NODE and TRIANGLE stay consistent under matrices that are a rotation only up to a part in 10^4, as stored poses
//          are.  A sheared or visibly scaled matrix is refused by the host.
// TRIANGLE (p0, e1, e2 of the hot record, in the instance's local frame.)  In the box frame: d0 = p0 - c_l, v0 = (a_k . d0), f1 = (a_k . e1),
//          f2 = (a_k . e2), v1 = v0 + f1, v2 = v0 + f2 — edges are projected, not end points, so roundings stay relative to the triangle's
//          size.  Then the 13-axis separating-axis test of Akenine-Möller (Fast 3D triangle-box overlap testing), every axis in the one form
//          "passes iff lo <= r and hi >= -r", lo / hi the reference min / max of the projected vertices, r the box's radius on that axis:
//            3 box axes        lo, hi over (v0.k, v1.k, v2.k), r = h_k
//            triangle normal   n = f1 x f2, lo = hi = n . v0, r = h.x |n.x| + (h.y |n.y| + h.z |n.z|)
//            9 cross axes      e_i x f for the box axes e_i and the edges f in (f1 on v0 opposite v2, f2 - f1 on v1 opposite v0, f2 on v0
//                              opposite v1): p = the projection of the edge's vertex and of the opposite one (the edge's other vertex projects
//                              to the same value), e.g. i = 0: p = f.y * v.z - f.z * v.y, r = h.y |f.z| + h.z |f.y|
//          The triangle OVERLAPS iff every axis passes; it is separated iff some axis separates strictly, so touching is overlapping.  A NaN
//          anywhere fails a comparison: a NaN never overlaps (the pad triangles of rtx_build_blas, NaN vertices — the normal axis reads all of
//          p0, e1, e2).  A zero-length cross axis or normal has p = 0 and r = 0 and passes: it never separates.
// SPHERE   (a surface, as everywhere in the query family.)  x_k = a_k . (centre - c), dmin2 = sum max(|x_k| - h_k, 0)^2 (the distance to the
//          box), dmax2 = sum (|x_k| + h_k)^2 (the distance to the farthest corner), both in the box frame; overlaps iff
//          dmin2 <= radius_squared and radius_squared <= dmax2.
// PLANE    overlaps iff |n.c + distance| <= h_0 |n.a_0| + (h_1 |n.a_1| + h_2 |n.a_2|).
// NODE     box against a node's AABB (mn, mx): TLAS nodes in world space, BLAS nodes in the instance's frame.  A conservative 6-axis test, no
//          cross axes, with m = (mn + mx) / 2, s = (mx - mn) / 2:
//            the coordinate axes j   c_j - E_j - pad <= mx_j and c_j + E_j + pad >= mn_j
//            the box axes k          |a_k . (m - c)| <= h_k + (s.x |a_k.x| + (s.y |a_k.y| + s.z |a_k.z|)) + pad
//          pad = ULPS * 2^-24 * (|c|_1 + |h|_1 + |m|_1 + |s|_1), |.|_1 the sum of the absolute components.  Roundings of one comparison: the two
//          halvings, m - c, a dot product, the radius, the sum: under 12 u of the magnitudes pad sums; the computed axes are unit and
//          orthogonal only to 25 u per axis (see MARGIN), which moves a projection of the box by under 50 u (|h|_1 + |m - c|).  ULPS = 64 covers
//          both for BLAS nodes.  A TLAS leaf's box was derived on the host or by rtx_update_instances from the instance's matrix with four more
//          roundings, and the instance's candidates are measured in its local frame: add the 8 u W of rtx_nearest_math.h's ACCURACY, taken over
//          the world magnitudes pad already sums: ULPS = 72 for TLAS nodes.  A node whose box truly intersects the query box is therefore never
//          rejected.  A NaN node box (a NaN pose) fails a comparison and is not entered, as in the other walks.
//          SPLIT LEAVES: a BLAS with spatial splits (the reference's SBVH) stores a triangle in several leaves, each slot under a box that
//          bounds only the part of the triangle inside that leaf.  NODE is conservative for the stored boxes, so such a slot is found where the
//          query box reaches its leaf's box; a slot of the same triangle under another leaf may stay unseen, as a slot of rtx_query_hits does
//          when the crossing lies in the other leaf.  Every TRIANGLE the box penetrates is still found through at least one of its slots.
// ORDER    overlaps are ordered by (object_id, triangle_id) ascending, ids in the public numberings of rtx_query_closest (instances, then
//          spheres, then planes; triangle_id = the triangle's slot in its BLAS, -1 for spheres and planes).  The list is the K smallest: it
//          depends only on WHICH overlaps the walk finds, never on the order of the walk or on the tree.  A BLAS whose leaves share triangles
//          (the spatial splits of the reference's SBVH) holds such a triangle once per slot, and every slot is an overlap of its own, as in
//          rtx_query_hits.
// WALK     (walk() below)  Spheres ascending, planes ascending, then the TLAS from its root.  A node is entered iff NODE passes (roots
//          included).  Of an inner node's two children the left one goes first and the right one, if it passes, is pushed: the node id alone,
//          no key, no second test when popped — there is no distance to order by and no bound that shrinks.  A TLAS leaf takes its instances in
//          tlas_indices order, stepped through in two registers, not on the stack; a BLAS leaf its slots in order.  STACK: a push happens only
//          at an inner node and leaves one sibling per level of the current path: at most rtxnp::stack_need() entries, by the argument of
//          rtx_nearest_math.h.  The caller checks it; there is no overflow path.
// FORMS    TRIANGLES  list and / or count of (object, slot) overlaps.
//          OBJECTS    list and / or count of distinct objects: an instance is left at its first overlapping slot and counted once.  An
//                     instance appears in exactly one TLAS leaf (the builders' invariant; overlap_check asserts it on its trees), so nothing
//                     else is needed to keep the objects distinct.  triangle ids are not reported.
//          ANY        0 or 1 per row: the lane leaves the walk at its first overlap.
// FILTER   (rtx_query_overlap_filtered)  The rule and the places of rtx_nearest_math.h's FILTER: a hidden sphere or plane is not tested, a
//          hidden instance is passed over at its TLAS leaf before its matrix is read, a row whose mask is 0 overlaps nothing, without a walk.
//          PROMISED then holds against the exhaustive search over the visible primitives.
// MARGIN   (margin() below) how far, as a distance, the computed triangle test may be from the exact one; u = 2^-24.  For one axis of the 13 the
//          GAP is the signed distance between the projections of box and triangle on the NORMALISED axis, positive when separated; the exact
//          test separates iff some gap is > 0.  S = |d0| + |e1| + |e2| + |h| (local scale), W = |c| + |c_l| (0 for an identity matrix, which is
//          exact).  Roundings on the path:
//            the axes: q / |q| 3.5 u per component, a matrix cell 8 u of its products and 3 u of its sums: a column is within 25 u of the exact
//              unit axis; xform_dir adds 3 u: a vector d projects with an error under 28 u |d| per component, 49 u |d| as a vector;
//            d0 = p0 - c_l: u |d0|;  c_l itself 4 u W, and the instance's stored matrix likewise: 8 u W, as rtx_nearest_math.h derives;
//            v1, v2: one more u each;  an axis evaluation (two or three products, the sums, r): under 4 u (|v| + |h|) of the NORMALISED axis,
//              whatever its direction — the cross axes' components are copies of f's, so p and r are exact up to those roundings;
//            the DIRECTION of a derived axis: f's components are off by 28 u |e|, n's by 59 u |f1||f2|: the axis turns by up to
//              102 u kappa, kappa = |f1||f2| / |n| for the normal and |f| / |e_i x f| for a cross axis (1 / the sine of the angle between the two
//              edges, resp. between the edge and the box axis), which moves a gap by that angle times (|v| + |h|); kappa = 1 for a box axis.
//          margin(S, W, kappa) = (192 S kappa + 8 W) u covers the sum.  What it states, per axis — the bound is normalised per axis, so an
//          ill-conditioned axis (an edge nearly parallel to a box axis, a sliver's normal) weakens only itself:
//            a triangle with SOME axis whose exact gap exceeds margin(S, W, that axis's kappa) is never reported;
//            a triangle whose every exact gap is below -margin(S, W, 1) — it penetrates deeper than that — is always reported: an axis in a
//              wrong direction is still an axis, and no direction separates two bodies that penetrate by more than its evaluation error.
//          Excluded: a gap that is positive only on axes with kappa beyond 2^10 (near-parallel edge / axis pairs), where the bound says
//          nothing useful; such a triangle may be reported although an exact test separates it.
// PROMISED   every listed overlap is an overlap of the exhaustive search (every primitive, no node tests, the same functions) with the same
//            bits, and count <= the exhaustive count; any == (count > 0); the objects form equals the distinct objects of the triangles form.
//            Because NODE is conservative, every primitive that penetrates by more than MARGIN is found — in a BLAS with split leaves through
//            at least one of its slots (SPLIT LEAVES above); the count of the exhaustive search, which tests every slot, is then larger.
// NOT PROMISED  equality with the exhaustive list for a primitive within MARGIN of touching: NODE's comparisons and TRIANGLE's are different
//            roundings of the same geometry, and a node test may reject a box whose triangle the triangle test accepts at a gap of 0.
// OUT OF SCOPE  convex hulls as query volumes (capsules and balls: rtx_capsule_math.h), penetration depth (swept boxes: rtx_boxsweep_math.h), or contact points, more than
//            RTX_QUERY_MAX_HITS entries per row, the rtx_group_* path.
#pragma once
#include <stdint.h>
#include "rtx_nearest_math.h"

namespace rtxop {

using rtxnp::P3;
using rtxnp::mk;
using rtxnp::add;
using rtxnp::sub;
using rtxnp::dot;
using rtxnp::ptr3;
using rtxnp::xform_pos;
using rtxnp::xform_dir;
using rtxnp::is_finite;

enum { MAX_HITS = 8, ROW_FLOATS = 10 };                        // RTX_QUERY_MAX_HITS
enum { FORM_TRIANGLES = 0, FORM_OBJECTS = 1, FORM_ANY = 2 };
enum { BLAS_ULPS = 64, TLAS_ULPS = 72 };                       // NODE's pad
RTX_HDF float min_ref(float a, float b) { return a < b ? a : b; }
RTX_HDF float max_ref(float a, float b) { return a > b ? a : b; }
RTX_HDF float mag(float f) { return __builtin_fabsf(f); }
RTX_HDF float unit_roundoff() { return 5.9604644775390625e-08f; }      // u = 2^-24
RTX_HDF P3 cross(P3 l, P3 r) { return mk(l.y * r.z - l.z * r.y, l.z * r.x - l.x * r.z, l.x * r.y - l.y * r.x); }
RTX_HDF float norm1(P3 a) { return mag(a.x) + (mag(a.y) + mag(a.z)); }

RTX_HDF bool row_is_live(const float * r) {
    for (int k = 0; k < ROW_FLOATS; k++) if (!is_finite(r[k])) return false;
    if (!((r[3] >= 0.0f) & (r[4] >= 0.0f) & (r[5] >= 0.0f))) return false;
    const float qq = r[6] * r[6] + (r[7] * r[7] + (r[8] * r[8] + r[9] * r[9]));
    return is_finite(qq) && qq > 0.0f;
}

// FRAME: the box as the tests read it, in world space or in an instance's local frame
struct Frame { P3 c, a0, a1, a2, h, E; float base; };          // base = |c|_1 + |h|_1, NODE's share of pad that belongs to the box

RTX_HDF void finish_frame(Frame & F) {
    const P3 g = mk(F.h.x / dot(F.a0, F.a0), F.h.y / dot(F.a1, F.a1), F.h.z / dot(F.a2, F.a2));
    F.E = mk(g.x * mag(F.a0.x) + (g.y * mag(F.a1.x) + g.z * mag(F.a2.x)),
             g.x * mag(F.a0.y) + (g.y * mag(F.a1.y) + g.z * mag(F.a2.y)),
             g.x * mag(F.a0.z) + (g.y * mag(F.a1.z) + g.z * mag(F.a2.z)));
    F.base = norm1(F.c) + norm1(F.h);
}
// the world frame of a LIVE row: the quaternion normalised, then rtxu::world_matrix's cells, the axes its columns
RTX_HDF Frame world_frame(const float * r) {
    Frame F;
    F.c = mk(r[0], r[1], r[2]); F.h = mk(r[3], r[4], r[5]);
    const float l = rtxnp::root(r[6] * r[6] + (r[7] * r[7] + (r[8] * r[8] + r[9] * r[9])));
    const float x = r[6] / l, y = r[7] / l, z = r[8] / l, w = r[9] / l;
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xz = x * z, xy = x * y, yz = y * z;
    const float wx = w * x, wy = w * y, wz = w * z;
    F.a0 = mk(1.0f - 2.0f * (yy + zz), 2.0f * (xy + wz),        2.0f * (xz - wy));            // cells 0, 4, 8
    F.a1 = mk(2.0f * (xy - wz),        1.0f - 2.0f * (xx + zz), 2.0f * (yz + wx));            // cells 1, 5, 9
    F.a2 = mk(2.0f * (xz + wy),        2.0f * (yz - wx),        1.0f - 2.0f * (xx + yy));     // cells 2, 6, 10
    finish_frame(F);
    return F;
}
RTX_HDF Frame local_frame(const Frame & W, const float * world_inv) {
    Frame F;
    F.c = xform_pos(world_inv, W.c);
    F.a0 = xform_dir(world_inv, W.a0); F.a1 = xform_dir(world_inv, W.a1); F.a2 = xform_dir(world_inv, W.a2);
    F.h = W.h;
    finish_frame(F);
    return F;
}
RTX_HDF P3 to_box(const Frame & F, P3 d) { return mk(dot(F.a0, d), dot(F.a1, d), dot(F.a2, d)); }

// one axis of TRIANGLE: passes iff lo <= r and hi >= -r
RTX_HDF bool axis_passes(float lo, float hi, float r) { return (lo <= r) & (hi >= -r); }
RTX_HDF bool axis_passes2(float pa, float pb, float r) { return axis_passes(min_ref(pa, pb), max_ref(pa, pb), r); }
// the three cross axes e_i x f of one edge: va a vertex of the edge, vb the opposite vertex
RTX_HDF bool edge_passes(P3 f, P3 va, P3 vb, P3 h) {
    const float ax = mag(f.x), ay = mag(f.y), az = mag(f.z);
    const bool p0 = axis_passes2(f.y * va.z - f.z * va.y, f.y * vb.z - f.z * vb.y, h.y * az + h.z * ay);
    const bool p1 = axis_passes2(f.z * va.x - f.x * va.z, f.z * vb.x - f.x * vb.z, h.x * az + h.z * ax);
    const bool p2 = axis_passes2(f.x * va.y - f.y * va.x, f.x * vb.y - f.y * vb.x, h.x * ay + h.y * ax);
    return p0 & p1 & p2;
}
RTX_HDF bool triangle_overlaps(const Frame & F, P3 p0, P3 e1, P3 e2) {
    const P3 v0 = to_box(F, sub(p0, F.c)), f1 = to_box(F, e1), f2 = to_box(F, e2);
    const P3 v1 = add(v0, f1), v2 = add(v0, f2), h = F.h;
    const bool bx = axis_passes(min_ref(min_ref(v0.x, v1.x), v2.x), max_ref(max_ref(v0.x, v1.x), v2.x), h.x);
    const bool by = axis_passes(min_ref(min_ref(v0.y, v1.y), v2.y), max_ref(max_ref(v0.y, v1.y), v2.y), h.y);
    const bool bz = axis_passes(min_ref(min_ref(v0.z, v1.z), v2.z), max_ref(max_ref(v0.z, v1.z), v2.z), h.z);
    const P3 n = cross(f1, f2);
    const float pn = dot(n, v0);
    const bool bn = axis_passes(pn, pn, h.x * mag(n.x) + (h.y * mag(n.y) + h.z * mag(n.z)));
    if (!(bx & by & bz & bn)) return false;
    const bool c1 = edge_passes(f1, v0, v2, h), c12 = edge_passes(sub(f2, f1), v1, v0, h), c2 = edge_passes(f2, v0, v1, h);
    return c1 & c12 & c2;
}
RTX_HDF bool sphere_overlaps(const Frame & F, P3 center, float radius_squared) {
    const P3 x = to_box(F, sub(center, F.c));
    const float ax = mag(x.x), ay = mag(x.y), az = mag(x.z);
    const float nx = max_ref(ax - F.h.x, 0.0f), ny = max_ref(ay - F.h.y, 0.0f), nz = max_ref(az - F.h.z, 0.0f);
    const float fx = ax + F.h.x, fy = ay + F.h.y, fz = az + F.h.z;
    const float dmin2 = nx * nx + (ny * ny + nz * nz), dmax2 = fx * fx + (fy * fy + fz * fz);
    return (dmin2 <= radius_squared) & (radius_squared <= dmax2);
}
RTX_HDF bool plane_overlaps(const Frame & F, P3 n, float distance) {
    const float s = dot(n, F.c) + distance;
    const float r = F.h.x * mag(dot(n, F.a0)) + (F.h.y * mag(dot(n, F.a1)) + F.h.z * mag(dot(n, F.a2)));
    return mag(s) <= r;
}
// NODE
RTX_HDF bool node_overlaps(const Frame & F, P3 mn, P3 mx, float ulps) {
    const P3 m = mk(0.5f * (mn.x + mx.x), 0.5f * (mn.y + mx.y), 0.5f * (mn.z + mx.z));
    const P3 s = mk(0.5f * (mx.x - mn.x), 0.5f * (mx.y - mn.y), 0.5f * (mx.z - mn.z));
    const float pad = (ulps * unit_roundoff()) * (F.base + (norm1(m) + norm1(s)));
    const bool cx = ((F.c.x - F.E.x) - pad <= mx.x) & ((F.c.x + F.E.x) + pad >= mn.x);
    const bool cy = ((F.c.y - F.E.y) - pad <= mx.y) & ((F.c.y + F.E.y) + pad >= mn.y);
    const bool cz = ((F.c.z - F.E.z) - pad <= mx.z) & ((F.c.z + F.E.z) + pad >= mn.z);
    const P3 t = sub(m, F.c);
    const bool b0 = mag(dot(F.a0, t)) <= (F.h.x + (s.x * mag(F.a0.x) + (s.y * mag(F.a0.y) + s.z * mag(F.a0.z)))) + pad;
    const bool b1 = mag(dot(F.a1, t)) <= (F.h.y + (s.x * mag(F.a1.x) + (s.y * mag(F.a1.y) + s.z * mag(F.a1.z)))) + pad;
    const bool b2 = mag(dot(F.a2, t)) <= (F.h.z + (s.x * mag(F.a2.x) + (s.y * mag(F.a2.y) + s.z * mag(F.a2.z)))) + pad;
    return cx & cy & cz & b0 & b1 & b2;
}

// ORDER: (object, triangle) ascending
RTX_HDF bool before(int32_t object, int32_t triangle, int32_t object2, int32_t triangle2) {
    if (object != object2) return object < object2;
    return triangle < triangle2;
}

RTX_HDF float margin(float local_scale, float world_scale, float kappa) { return (192.0f * local_scale * kappa + 8.0f * world_scale) * unit_roundoff(); }

// what a row's walk keeps: the overlaps seen, the entries the list holds
struct Tally { int32_t count, held; };

// One overlap.  List gives get(j, object, triangle) and set(j, object, triangle) for entries 0 .. K - 1.  A sorted insert over at most K entries;
// the loop bound is K, the same for every lane.  K == 0: count only.
template <typename List>
RTX_HDF void offer(List & L, const int K, Tally & w, const int32_t object, const int32_t triangle) {
    w.count++;
    if (K <= 0) return;
    int e = w.held;                                                        // the entry the overlap starts at, before it moves forward
    if (w.held == K) {
        int32_t lo, ls;
        L.get(K - 1, lo, ls);
        if (!before(object, triangle, lo, ls)) return;
        e = K - 1;
    } else w.held++;
    bool placed = false;
    for (int j = K - 1; j > 0; j--) {
        if (!placed && j <= e) {
            int32_t po, ps;
            L.get(j - 1, po, ps);
            if (before(object, triangle, po, ps)) L.set(j, po, ps);
            else { L.set(j, object, triangle); placed = true; }
        }
    }
    if (!placed) L.set(0, object, triangle);
}

// spheres and planes of a live row: the first step of the walk, and of the exhaustive search; true: an ANY row is answered
template <int FORM, typename Scene, typename List>
RTX_HDF bool world_primitives(Scene & sc, List & L, const int K, Tally & w, const Frame & W) {
    const int32_t ic = sc.instance_count(), sn = sc.sphere_count();
    for (int i = 0; i < sn; i++) {
        if (!sc.sphere_visible(i)) continue;
        P3 c; float r2;
        sc.sphere(i, c, r2);
        if (sphere_overlaps(W, c, r2)) { offer(L, K, w, ic + i, -1); if (FORM == FORM_ANY) return true; }
    }
    for (int i = 0; i < sc.plane_count(); i++) {
        if (!sc.plane_visible(i)) continue;
        P3 n; float dist;
        sc.plane(i, n, dist);
        if (plane_overlaps(W, n, dist)) { offer(L, K, w, ic + sn + i, -1); if (FORM == FORM_ANY) return true; }
    }
    return false;
}

// The walk.  Scene gives the records as for rtxnp::walk, plus instance_count() and enter(slot, F) (makes the BLAS of instance
// tlas_indices[slot] current, turns the world frame F into that instance's local frame, returns that instance) and FILTER's predicates.
// Stack gives push(sp, node) and pop(sp, node).  One frame is held: the world frame is made again from the row when an instance is done
// (the same function of the same floats: the same bits), so `row` must stay readable during the walk.
template <int FORM, typename Scene, typename Stack, typename List>
RTX_HDF void walk(Scene & sc, Stack & st, List & L, const float * row, const int K, Tally & w) {
    w.count = 0; w.held = 0;
    if (!row_is_live(row) || !sc.row_visible()) return;
    Frame F = world_frame(row);
    if (world_primitives<FORM>(sc, L, K, w, F)) return;
    if (sc.tlas_nodes() <= 0) return;
    int sp = 0, floor_sp = 0, cur = -1, first = 0, count = 0, tl_i = 0, tl_end = 0, inst = 0;
    bool in_blas = false;
    { P3 mn, mx; sc.tlas_node(0, mn, mx, first, count); if (node_overlaps(F, mn, mx, (float)TLAS_ULPS)) cur = 0; }
    for (;;) {
        if (cur < 0) {
            if (in_blas && sp == floor_sp) { in_blas = false; F = world_frame(row); }                           // this instance is done: back to world space
            if (!in_blas && tl_i < tl_end) {                                                      // the next instance of the TLAS leaf
                if (!sc.instance_visible(tl_i)) { tl_i++; continue; }                             // FILTER: hidden from this row
                inst = sc.enter(tl_i++, F);
                P3 mn, mx; sc.blas_node(0, mn, mx, first, count);
                in_blas = true; floor_sp = sp;
                if (node_overlaps(F, mn, mx, (float)BLAS_ULPS)) cur = 0;
                continue;
            }
            if (sp == 0) break;
            sp--; st.pop(sp, cur);
            P3 mn, mx;
            if (in_blas) sc.blas_node(cur, mn, mx, first, count); else sc.tlas_node(cur, mn, mx, first, count);
        }
        if ((count & 0x3fffffff) > 0) {                                                           // a leaf: (first, count) of node cur
            const int n = count & 0x3fffffff;
            cur = -1;
            if (in_blas) {
                for (int i = first; i < first + n; i++) {
                    P3 p0, e1, e2;
                    sc.triangle(i, p0, e1, e2);
                    if (!triangle_overlaps(F, p0, e1, e2)) continue;
                    if (FORM == FORM_TRIANGLES) { offer(L, K, w, inst, i); continue; }
                    offer(L, K, w, inst, -1);
                    if (FORM == FORM_ANY) return;
                    sp = floor_sp;                                                                // OBJECTS: this instance is counted, leave it
                    break;
                }
            } else { tl_i = first; tl_end = first + n; }
            continue;
        }
        P3 lmn, lmx, rmn, rmx; int lf, lc, rf, rc;
        const int left = first;
        if (in_blas) { sc.blas_node(left, lmn, lmx, lf, lc); sc.blas_node(left + 1, rmn, rmx, rf, rc); }
        else         { sc.tlas_node(left, lmn, lmx, lf, lc); sc.tlas_node(left + 1, rmn, rmx, rf, rc); }
        const float ulps = in_blas ? (float)BLAS_ULPS : (float)TLAS_ULPS;
        const bool pl = node_overlaps(F, lmn, lmx, ulps), pr = node_overlaps(F, rmn, rmx, ulps);
        if (pl && pr) { st.push(sp, left + 1); sp++; }
        if (pl) { cur = left; first = lf; count = lc; }
        else if (pr) { cur = left + 1; first = rf; count = rc; }
        else cur = -1;
    }
}

}  // namespace rtxop
