// rtx_capsule_math.h — the arithmetic AND the walk of capsule-overlap queries (include/rtx.h: rtx_query_overlap_capsule), written once and
// compiled twice like rtx_overlap_math.h: by hipcc into k_query_overlap_capsule (rtx_capsule.h) and by the host compiler into
// rtxh_query_overlap_capsule / rtxh_query_overlap_capsule_exhaustive (host/rtx_host.cpp) and capsule_check.cpp.  Unfused fp32
// (-ffp-contract=off), correctly rounded '/' and sqrtf on both sides, every sum of three products in vdot's order x + (y + z);
// min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b (a NaN gives b).  So every function here returns the same bits on the CPU and on
// gfx950.  Plain C++: no HIP types.  This comment is the specification.
//
// ROW      seven floats: start point p (3), axis vector d (3), radius r.  The capsule is every point within r of the segment p + s d,
//          s in [0, 1].  A row is LIVE when all seven floats are finite and r >= 0.  d == 0 is a ball, r == 0 a segment, both a point: all
//          valid.  A dead row overlaps nothing, has count 0 and an empty list, and is not walked.  Why (p, d, r) and not two end points: the
//          axis is taken into an instance's frame as a vector (xform_dir), as rtx_overlap_math.h's TRIANGLE projects a triangle's edges and
//          not its end points, so roundings stay relative to the capsule's size; the rows are the first seven floats of a rtx_query_sweep row
//          with d = direction * D; and the ray sort key of the ray queries applies unchanged.
// FRAME    what the tests read: p, d, r.  In an instance's local frame p_l = xform_pos(world_inv, p), d_l = xform_dir(world_inv, d), r
//          unchanged: exact for a rigid pose, the only kind the host lets through (the rigid rule of rtx_query_nearest).  Relative to a
//          triangle m = p_l - p0.
// TRIANGLE (p0, e1, e2 of the hot record, in the instance's local frame; m = p_l - p0, d = d_l, rr = r * r.)  The triangle OVERLAPS iff
//          dist(segment, triangle) <= r; touching overlaps.  In this order, the first that decides:
//            guard     g = m.m + (e1.e1 + e2.e2); not (g >= 0) — a NaN anywhere — never overlaps (the pad triangles of rtx_build_blas, NaN
//                      vertices).  A degenerate triangle is the union of its edges and is tested as that.
//            bounds    per coordinate j: lo = min(m_j, m_j + d_j) - r, hi = max(m_j, m_j + d_j) + r, against tlo = min(min(e1_j, e2_j), 0),
//                      thi = max(max(e1_j, e2_j), 0): not (lo <= thi and hi >= tlo) on some j: no overlap.  Conservative, no kappa.
//            ends      triangle_d2(m, e1, e2) <= rr or, when d != 0, triangle_d2(m + d, e1, e2) <= rr (rtx_nearest_math.h's TRIANGLE): overlap.
//                      d.d == 0 (a ball): nothing else is tested — the edges are part of the triangle.
//            pierce    Möller–Trumbore without its division: pv = d x e2, det = e1.pv, u = m.pv, qv = m x e1, v = d.qv, t = e2.qv; with
//                      the sign of det taken out of u, v, t: det * det > 2^-20 ((d.d) (e1.e1)) (e2.e2) (kappa below 2^10: see THE PITFALL),
//                      u >= 0, v >= 0, u + v <= |det| and 0 < t < |det| (the end points lie strictly on opposite sides of the plane and
//                      the crossing point is inside the triangle): distance 0, overlap.
//            edges     the segment against the edges (0, e1), (0, e2), (e1, e2 - e1) as clamped segment-segment closest points (Ericson,
//                      Real-Time Collision Detection 5.1.9), segment_d2() below: with w = m - q (q the edge's start, f its vector),
//                      a = d.d (> 0 here), e = f.f, c = d.w, g = f.w, b = d.f, den = a e - b b:
//                        e == 0 (a point)  t = 0, s = clamp(-c / a)
//                        otherwise         s = den != 0 ? clamp((b g - c e) / den) : 0;  t = (b s + g) / e;
//                                          t < 0: t = 0, s = clamp(-c / a);   t > 1: t = 1, s = clamp((b - c) / a)
//                      clamp(x) = min(max(x, 0), 1); x = w + (d s - f t) per component, d2 = x.x; d2 <= rr on some edge: overlap.
//          THE PITFALL of the interior parameter: den is all rounding for a near-parallel pair.  Because t is derived again from the clamped
//          s, and s again from a clamped t, both points lie ON their segments whatever s is: the computed distance is never below the true
//          one by more than its own roundings.  It can be above it by about u kappa |d|, kappa = |d||f| / |d x f| (1 / the sine of the angle
//          between the pair) — the kappa rtx_overlap_math.h's cross axes have — and by no more than |d| / kappa, what a wrong s can cost
//          between two nearly parallel lines.  pierce has its own: kappa = |d||e1||e2| / |det|, the quotient against the plane.  With det
//          all rounding (a segment nearly in the triangle's plane) the signs of u, v, t are rounding too and pierce would report
//          triangles the segment passes at a distance: it is not evaluated beyond kappa = 2^10, where ends and edges decide alone.
// SPHERE   (a shell, as everywhere in the query family.)  v = p - centre, a = d.d, s = a > 0 ? clamp(-(d.v) / a) : 0, q = v + d s,
//          dmin = sqrtf(q.q) (centre to segment), dmax = max(sqrtf(v.v), sqrtf(w.w)), w = v + d (the farther end point),
//          R = sqrtf(radius_squared); overlaps iff dmin <= R + r and dmax + r >= R.  A capsule strictly inside the ball does not overlap.
// PLANE    sa = n.p + distance, sb = n.(p + d) + distance; overlaps iff min(sa, sb) <= r and max(sa, sb) >= -r.
// NODE     capsule against a node's AABB (mn, mx): TLAS nodes in world space, BLAS nodes in the instance's frame.  Conservative and
//          division-free (no slab quotients: a zero component of d needs no special case and no 0 * inf appears): the segment-against-AABB
//          separating-axis test (Ericson 5.3.3) with the box inflated by r, which contains the true Minkowski sum and is loose only near
//          corners.  n = (mn + mx) / 2, s = (mx - mn) / 2, h = d / 2 (exact), k = p + h the midpoint, c = k - n, A_j = |k_j| + |n_j|:
//            3 coordinate axes   |c_j| <= (s_j + (r + |h_j|)) + pad,         pad = ULPS u (A_j + (s_j + (r + |h_j|)))
//            3 cross axes        |c_y h_z - c_z h_y| <= (s_y |h_z| + s_z |h_y|) + (r (|h_y| + |h_z|) + pad), cyclic,
//                                pad = ULPS u ((A_y |h_z| + A_z |h_y|) + ((s_y |h_z| + s_z |h_y|) + r (|h_y| + |h_z|)))
//          The cross axis e_j x h has length sqrtf(h_y^2 + h_z^2) <= |h_y| + |h_z|: the sum stands for it, so no root is taken and the
//          test stays conservative.  pad is ULPS u times the sum of the magnitudes that enter the comparison — those of k and n, not of
//          their difference, which may cancel.  Roundings of one comparison: the two halvings' sums (u each), k (u), c (u): 3 u A_j in c;
//          a product and the difference of a cross axis 2 u; the right side three products and three sums: all under 8 u of what pad sums.
//          ULPS = 16 for BLAS nodes doubles that.  A TLAS leaf's box was derived from the instance's matrix with four more roundings and
//          the instance's candidates are measured in its local frame: add the 8 u W of rtx_nearest_math.h's ACCURACY, taken over the world
//          magnitudes pad already sums: ULPS = 24 for TLAS nodes.  A node whose box truly meets the capsule is therefore never rejected.  A
//          NaN node box (a NaN pose) fails a comparison and is not entered.  A ball (h = 0) is a point against the inflated box: the cross
//          axes read 0 <= pad.  SPLIT LEAVES: the note of rtx_overlap_math.h applies unchanged.
// ORDER    overlaps are ordered by (object_id, triangle_id) ascending, ids in the public numberings of rtx_query_closest; the list is the K
//          smallest, through rtxop::offer / before / Tally: it depends only on WHICH overlaps the walk finds.
// WALK     (walk() below)  rtx_overlap_math.h's: spheres ascending, planes ascending, then the TLAS from its root; a node is entered iff
//          NODE passes (roots included); the left child first, the right one, if it passes, pushed as a node id alone; a TLAS leaf's
//          instances stepped through in two registers; at most rtxnp::stack_need() entries, checked by the caller.
// FORMS    TRIANGLES, OBJECTS (an instance is left at its first overlapping slot and counted once), ANY (the lane leaves the walk at its
//          first overlap): rtx_overlap_math.h's.
// FILTER   (rtx_query_overlap_capsule_filtered)  rtx_nearest_math.h's FILTER: a hidden sphere or plane is not tested, a hidden instance is
//          passed over at its TLAS leaf before its matrix is read, a row whose mask is 0 overlaps nothing, without a walk.
// MARGIN   (margin() below) how far, as a distance, the computed triangle test may be from the exact one; u = 2^-24.
//          S = |m| + |d| + |e1| + |e2| + r (local scale), W = |p| + |p_l| (0 for an identity matrix, which is exact).  Roundings on the path:
//            p_l 4 u W and the instance's stored matrix likewise: 8 u W, as rtx_nearest_math.h derives;  d_l: 3 u |d| per component, under
//              6 u |d| as a vector;  m = p_l - p0: u |m|;  m + d: u more;  rr and the comparison with it: u of r, 1.5 u of the distance;
//            bounds: two roundings per side, 2 u S: no kappa;
//            ends: 16 u S (candidate_error of rtx_nearest_math.h) on top of the above: under 26 u S;
//            edges: the point x = w + (d s - f t): w u, two products and two sums per component, 4 u (|w| + |d| + |f|), under 7 u S as a
//              vector, x.x 1.5 u of the distance: with the above under 17 u S BELOW the truth, whatever s and t are; above it by the
//              parameters' error: the five dot products 3 u each, den 2 u more of a e, the quotients u: under 12 u kappa of a parameter, which
//              moves a point by 12 u kappa |d| along a segment and the distance by no more: under (17 + 12 kappa) u S;
//            pierce: pv, qv 2 u of their products per component, d_l's 6 u in pv and v; det, u, v, t 3 u more each: each within
//              12 u |d||e1||e2| (|m| for an edge where it enters), so the crossing point lies within 12 u kappa (|m| + |e1| + |e2|) of
//              where the inequalities put it, u + v <= |det| with two of them and a sum: under 48 u kappa S.
//          margin(S, W, kappa) = (C S kappa + 8 W) u with C = 64 covers the largest of these sums (48 kappa, 29 kappa at kappa >= 1).  What it
//          states:
//            a triangle whose exact distance to the segment exceeds r + margin(S, W, kappa) is never reported, kappa that of the sub-test
//              that would have reported it (1 for ends);
//            a triangle whose exact distance is below r - margin(S, W, 1) is always reported, the closest pair being well conditioned.
//          Excluded, as in rtx_overlap_math.h: decisions that rest only on a pair with kappa beyond 2^10 (a segment nearly parallel to
//          an edge whose closest points are interior to both; a segment nearly in the triangle's plane that crosses it is found only
//          through ends and edges, so not at a radius below their margin).
// PROMISED   every listed overlap is an overlap of the exhaustive search (every primitive, no node tests, the same functions) with the
//            same bits, and count <= the exhaustive count; any == (count > 0); the objects form equals the distinct objects of the
//            triangles form.  Because NODE is conservative, every primitive closer than r - MARGIN is found — in a BLAS with split leaves
//            through at least one of its slots.
// NOT PROMISED  equality with the exhaustive list for a primitive within MARGIN of touching: NODE's comparisons and TRIANGLE's are
//            different roundings of the same geometry.
// OUT OF SCOPE  swept capsules (a ball: rtx_sweep_math.h), a contact point or penetration depth, a position sort key for ball-only batches,
//            more than RTX_QUERY_MAX_HITS entries per row, the rtx_group_* path.
#pragma once
#include <stdint.h>
#include "rtx_overlap_math.h"

namespace rtxcp {

using rtxnp::P3;
using rtxnp::mk;
using rtxnp::add;
using rtxnp::sub;
using rtxnp::dot;
using rtxnp::scale;
using rtxnp::xform_pos;
using rtxnp::xform_dir;
using rtxnp::is_finite;
using rtxop::min_ref;
using rtxop::max_ref;
using rtxop::mag;
using rtxop::cross;
using rtxop::unit_roundoff;
using rtxop::offer;
using rtxop::Tally;

enum { MAX_HITS = rtxop::MAX_HITS, ROW_FLOATS = 7, KEY_FLOATS = 6 };
enum { FORM_TRIANGLES = rtxop::FORM_TRIANGLES, FORM_OBJECTS = rtxop::FORM_OBJECTS, FORM_ANY = rtxop::FORM_ANY };
enum { BLAS_ULPS = 16, TLAS_ULPS = 24 };                       // NODE's pad

RTX_HDF float clamp01(float x) { return min_ref(max_ref(x, 0.0f), 1.0f); }

RTX_HDF bool row_is_live(const float * r) {
    for (int k = 0; k < ROW_FLOATS; k++) if (!is_finite(r[k])) return false;
    return r[6] >= 0.0f;
}

// FRAME: the capsule as the tests read it, in world space or in an instance's local frame
struct Frame { P3 p, d; float r; };

RTX_HDF Frame world_frame(const float * r) { Frame F; F.p = mk(r[0], r[1], r[2]); F.d = mk(r[3], r[4], r[5]); F.r = r[6]; return F; }
RTX_HDF Frame local_frame(const Frame & W, const float * world_inv) {
    Frame F;
    F.p = xform_pos(world_inv, W.p); F.d = xform_dir(world_inv, W.d); F.r = W.r;
    return F;
}

// edges of TRIANGLE: the squared distance between the segment w + d s (relative to the edge's start) and the edge f t; a = d.d > 0
RTX_HDF float segment_d2(P3 w, P3 d, float a, P3 f) {
    const float e = dot(f, f), c = dot(d, w);
    float s, t;
    if (e == 0.0f) { t = 0.0f; s = clamp01(-c / a); }
    else {
        const float g = dot(f, w), b = dot(d, f);
        const float den = a * e - b * b;
        s = den != 0.0f ? clamp01((b * g - c * e) / den) : 0.0f;
        t = (b * s + g) / e;
        if (t < 0.0f) { t = 0.0f; s = clamp01(-c / a); }
        else if (t > 1.0f) { t = 1.0f; s = clamp01((b - c) / a); }
    }
    const P3 x = mk(w.x + (d.x * s - f.x * t), w.y + (d.y * s - f.y * t), w.z + (d.z * s - f.z * t));
    return dot(x, x);
}
RTX_HDF bool bounds_pass(float ma, float da, float r, float ea, float eb) {
    const float mb = ma + da;
    const float lo = min_ref(ma, mb) - r, hi = max_ref(ma, mb) + r;
    const float tlo = min_ref(min_ref(ea, eb), 0.0f), thi = max_ref(max_ref(ea, eb), 0.0f);
    return (lo <= thi) & (hi >= tlo);
}
RTX_HDF bool triangle_overlaps(const Frame & F, P3 p0, P3 e1, P3 e2) {
    const P3 m = sub(F.p, p0), d = F.d;
    const float r = F.r, rr = r * r;
    const float g = dot(m, m) + (dot(e1, e1) + dot(e2, e2));
    if (!(g >= 0.0f)) return false;
    if (!(bounds_pass(m.x, d.x, r, e1.x, e2.x) & bounds_pass(m.y, d.y, r, e1.y, e2.y) & bounds_pass(m.z, d.z, r, e1.z, e2.z))) return false;
    float u, v;
    if (rtxnp::triangle_d2(m, e1, e2, u, v) <= rr) return true;
    const float a = dot(d, d);
    if (a == 0.0f) return false;
    if (rtxnp::triangle_d2(add(m, d), e1, e2, u, v) <= rr) return true;
    {   // pierce
        const P3 pv = cross(d, e2), qv = cross(m, e1);
        float det = dot(e1, pv), bu = dot(m, pv), bv = dot(d, qv), bt = dot(e2, qv);
        if (det < 0.0f) { det = -det; bu = -bu; bv = -bv; bt = -bt; }
        if ((det * det > 9.5367431640625e-07f * ((a * dot(e1, e1)) * dot(e2, e2))) & (bu >= 0.0f) & (bv >= 0.0f) & (bu + bv <= det) & (bt > 0.0f) & (bt < det)) return true;
    }
    if (segment_d2(m, d, a, e1) <= rr) return true;
    if (segment_d2(m, d, a, e2) <= rr) return true;
    return segment_d2(sub(m, e1), d, a, sub(e2, e1)) <= rr;
}
RTX_HDF bool sphere_overlaps(const Frame & F, P3 center, float radius_squared) {
    const P3 v = sub(F.p, center), w = add(v, F.d);
    const float a = dot(F.d, F.d);
    const float s = a > 0.0f ? clamp01(-dot(F.d, v) / a) : 0.0f;
    const P3 q = add(v, scale(F.d, s));
    const float dmin = rtxnp::root(dot(q, q)), dmax = max_ref(rtxnp::root(dot(v, v)), rtxnp::root(dot(w, w)));
    const float R = rtxnp::root(radius_squared);
    return (dmin <= R + F.r) & (dmax + F.r >= R);
}
RTX_HDF bool plane_overlaps(const Frame & F, P3 n, float distance) {
    const float sa = dot(n, F.p) + distance, sb = dot(n, add(F.p, F.d)) + distance;
    return (min_ref(sa, sb) <= F.r) & (max_ref(sa, sb) >= -F.r);
}
// NODE
RTX_HDF bool node_axis(float c, float A, float s, float rh, float uu) { return mag(c) <= (s + rh) + uu * (A + (s + rh)); }
RTX_HDF bool node_cross(float ca, float cb, float Aa, float Ab, float sa, float sb, float ha, float hb, float r, float uu) {
    // the axis with components (a, b) of c, A, s and |h|: |c_a h_b - c_b h_a|, ha and hb signed
    const float ma = mag(ha), mb = mag(hb);
    const float box = sa * mb + sb * ma, cap = r * (ma + mb);
    return mag(ca * hb - cb * ha) <= box + (cap + uu * ((Aa * mb + Ab * ma) + (box + cap)));
}
RTX_HDF bool node_overlaps(const Frame & F, P3 mn, P3 mx, float ulps) {
    const P3 n = mk(0.5f * (mn.x + mx.x), 0.5f * (mn.y + mx.y), 0.5f * (mn.z + mx.z));
    const P3 s = mk(0.5f * (mx.x - mn.x), 0.5f * (mx.y - mn.y), 0.5f * (mx.z - mn.z));
    const P3 h = mk(0.5f * F.d.x, 0.5f * F.d.y, 0.5f * F.d.z);
    const P3 k = add(F.p, h), c = sub(k, n);
    const P3 A = mk(mag(k.x) + mag(n.x), mag(k.y) + mag(n.y), mag(k.z) + mag(n.z));
    const float uu = ulps * unit_roundoff(), r = F.r;
    const bool a0 = node_axis(c.x, A.x, s.x, r + mag(h.x), uu), a1 = node_axis(c.y, A.y, s.y, r + mag(h.y), uu), a2 = node_axis(c.z, A.z, s.z, r + mag(h.z), uu);
    const bool x0 = node_cross(c.y, c.z, A.y, A.z, s.y, s.z, h.y, h.z, r, uu);
    const bool x1 = node_cross(c.z, c.x, A.z, A.x, s.z, s.x, h.z, h.x, r, uu);
    const bool x2 = node_cross(c.x, c.y, A.x, A.y, s.x, s.y, h.x, h.y, r, uu);
    return a0 & a1 & a2 & x0 & x1 & x2;
}

RTX_HDF float margin(float local_scale, float world_scale, float kappa) { return (64.0f * local_scale * kappa + 8.0f * world_scale) * unit_roundoff(); }

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

// The walk: rtxop::walk over this header's Frame and tests.  Scene, Stack and List as there; enter(slot, F) turns the world frame F into
// the local frame of instance tlas_indices[slot].  One frame is held: the world frame is made again from the row when an instance is done,
// so `row` must stay readable during the walk.
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

}  // namespace rtxcp
