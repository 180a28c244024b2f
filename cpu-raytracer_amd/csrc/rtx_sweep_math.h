// rtx_sweep_math.h — the arithmetic AND the walk of swept-sphere queries (include/rtx.h: rtx_query_sweep), written once and compiled twice
// like rtx_nearest_math.h and rtx_hits_math.h, whose functions it reuses: by hipcc into k_query_sweep (rtx_sweep.h) and by the host compiler
// into rtxh_query_sweep / rtxh_query_sweep_exhaustive (host/rtx_host.cpp) and sweep_check.cpp.  Unfused fp32 (-ffp-contract=off), correctly
// rounded '/' and sqrtf on both sides, every sum of three products in vdot's order x + (y + z); min(a, b) = a < b ? a : b and
// max(a, b) = a > b ? a : b.  So every function here returns the same bits on the CPU and on gfx950.  Plain C++: no HIP types.  This
// comment is the specification.
//
// ROW      (ox, oy, oz, dx, dy, dz, D, r): a ball of radius r (world units) whose centre moves along c(t) = o + t * d, d as given, t in units
//          of |d|.  A row is LIVE when its first seven floats are a live row of rtx_hits_math.h (direction not (+-0, +-0, +-0), six finite
//          components, D > 0, +INFINITY included) and r is finite and > 0.  A dead row gets the no-answer record and is not walked.
// ANSWER   the smallest t in [0, D) at which the distance from c(t) to the surface rtx_query_nearest measures (two-sided triangles, sphere
//          shells, two-sided planes) is <= r.  Every primitive yields at most one CANDIDATE (t, d20): its first contact time, and its squared
//          distance from o as rtx_nearest_math.h computes it.  A primitive within r of o is an OVERLAP candidate: t = 0.  Candidates are
//          ordered by (t, d20) ascending; t < D is strict.  So a row that overlaps at its origin reports the primitive and the surface point
//          rtx_query_nearest reports for (o, r).  An exact tie in both goes to the lowest (kind, object, slot), kinds in the order sphere,
//          plane, triangle: the first the exhaustive search finds, and among the candidates offered the same one whatever order a tree is
//          walked in (two triangles that share the edge or the vertex a ball meets head-on tie exactly).  WHICH triangles offer a candidate
//          depends on the order by the plane early-out below, within its rounding.
// ROOTS    every quadratic is solved from the closest approach, never as b^2 - 4ac from the origin (which loses a small ball far away to
//          cancellation).  approach(m, d, q2): tc = -(m.d) / (d.d), k = m + d * tc, w = (q2 - k.k) / (d.d); no contact unless w >= 0 (a NaN
//          is none); sq = sqrtf(w).  entry_time: t = tc - sq; a negative t becomes 0 when tc + sq >= 0 (the origin is inside by a rounding:
//          the overlap test has looked already) and is no contact otherwise.
// TRIANGLE (p0, e1, e2) of the hot record in the instance's local ray: co = xform_pos(world_inv, o), cd = xform_dir(world_inv, d) as in
//          rtx_hits_math.h, r unchanged (local units: the host lets rigid poses through only).  m = co - p0, n = e1 x e2.  In this order:
//   plane    h = n.m, g = n.cd, rn = r * sqrtf(n.n).  If |h| > rn the ball starts outside the plane's slab: s = h > 0 ? -g : g is its
//            speed towards it; no candidate unless s > 0; tp = (|h| - rn) / s; no candidate unless tp <= bound (the walk's current best t:
//            nothing of this triangle is reached earlier than its slab).  Otherwise tp = 0.  Most triangles of a leaf end here.
//            ORDER  in exact arithmetic no contact of the triangle is earlier than tp; the computed t of a rim contact can round below the
//            computed tp (by ulps head-on; by more in t, though not in distance, where the ball grazes the plane: tp divides a rounded
//            |h| - rn by a small s).  Such a triangle, called again with bound = its own t, yields no candidate.  So whether it competes
//            depends on the candidates seen before it: the early-out's order dependence is part of the specification.  Raising the rim's t
//            to tp instead would put a grazing ball past the rim by far more than the bound.  What it costs is covered by ACCURACY: a
//            triangle passed over had its slab, so itself, no nearer than r minus the early-out's rounding at the bound.
//   overlap  d20 = rtxnp::triangle_d2(m, e1, e2, u, v); if d20 <= r * r the candidate is (0, d20) at those weights.
//   settled  if bound == 0 (the answer is at t = 0 already) and d20 > the answer's d20, no candidate: whatever the face or a rim gave
//            would lose by ANSWER's order.  (Not "bound == 0" alone: an answer at t = 0 may be a rim contact that entry_time raised to 0,
//            with a d20 above r * r, and a nearer one of the same kind must still win.)  It changes no answer, only the work.
//   face     c = m + cd * tp; with aa = e1.e1, ab = e1.e2, cc = e2.e2, d1 = e1.c, d2 = e2.c, det = aa * cc - ab * ab:
//            u = (cc * d1 - ab * d2) / det, v = (aa * d2 - ab * d1) / det; if u >= 0, v >= 0 and u + v <= 1 the candidate is (tp, d20) at (u, v).
//            (A ball inside the slab and off the triangle never reaches the face first: tp = 0 only catches an overlap lost to rounding.)
//   rims     otherwise the earliest of, in this order, a later one only if strictly earlier: the edge cylinders (p0, e1) -> (s, 0),
//            (p0, e2) -> (0, s), (p0 + e1, e2 - e1) -> (1 - s, s), then the vertex spheres p0 -> (0, 0), p0 + e1 -> (1, 0), p0 + e2 -> (0, 1).
//            Edge (a, e), ma = co - a: fm = (ma.e) / (e.e), fd = (cd.e) / (e.e), the parts across the edge mp = ma - e * fm,
//            dp = cd - e * fd; entry_time(approach(mp, dp, r * r)) gives t; s = fm + t * fd must lie in [0, 1].  Vertex a:
//            entry_time(approach(co - a, cd, r * r)).  A zero edge, a motion along an edge, a NaN: every comparison is false, no candidate.
// SPHERE   centre c, R = sqrtf(radius_squared): m = o - c, l = sqrtf(m.m), s = l - R, d20 = s * s.  Overlap iff |s| <= r.  From outside
//          (s > 0) entry_time(approach(m, d, (R + r)^2)).  From inside the shell the exit root against R - r: t = tc + sqrtf(max(w, 0)),
//          a negative t is 0 (the ball is inside and must come out).
// PLANE    s = n.o + distance, d20 = s * s.  Overlap iff |s| <= r.  Else g = n.d, a = s > 0 ? -g : g, a candidate iff a > 0: t = (|s| - r) / a.
// OUTPUTS  distance = t.  With cc = t == 0 ? o : o + d * t, the centre at the contact: a sphere or a plane reports rtxnp::sphere_outputs /
//          plane_outputs at cc; a triangle reports position = xform_pos(world, p0 + (e1 * u + e2 * v)) and normal, uv by
//          rtxnp::triangle_outputs at (u, v): what rtx_query_nearest reports for that surface point, ids in its numberings.  The geometric
//          contact normal is (cc - position) / r.  No answer: distance +inf, floats 0, ids -1.
//
// THE WALK (walk() below; part of the specification)
//   1. bound = D.  A candidate with t < D replaces the answer when it is before it in ANSWER's order; bound = the answer's t.
//   2. Spheres ascending, planes ascending, then the TLAS from its root.
//   3. While the answer is no overlap (none yet, or t > 0) a node is entered iff slab(): g = r + slack (below); per axis
//      t0 = ((min - g) - o) * inv, t1 = ((max + g) - o) * inv, inv = 1 / d per component, key = max(max(0, tmin.x), max(tmin.y, tmin.z)),
//      exit = min(tmax.x, min(tmax.y, tmax.z)); pass iff key <= exit and key <= bound.  A NaN (an origin on a grown box plane, moving along
//      it) passes nothing.
//   4. Once the answer has t == 0 a node is entered iff key = rtxnp::box_d2(origin, box) <= lim * lim, lim = sqrtf(the answer's d20) + slack:
//      the rest of the walk is the nearest-point walk of rtx_nearest_math.h.
//      SLACK  sigma = max(|min.x - o.x|, |max.x - o.x|) + the same of y + the same of z bounds the distance from the origin to anything in
//      the box, and 2 sigma each edge of a triangle inside it, so S <= 5 sigma and T <= sigma + r for every candidate of the subtree.  With
//      ACCURACY's candidate_error <= (130 sigma + 14 r) u and the test's own roundings (two differences, an inverse and a product per plane:
//      4u (sigma + r); 2.5u of the box distance) slack = (160 sigma + 32 r) * 2^-24 makes the test conservative against the COMPUTED
//      candidates: a BLAS subtree is skipped only if no triangle in it yields a candidate at or before the answer.  So within one instance
//      the walk returns what the search over all its triangles returns, up to the plane early-out's ORDER: the two meet the triangles in
//      different orders, and a triangle whose t rounds below its own tp competes in one and not in the other.  Then their t differ within
//      that rounding, either way round; both satisfy ACCURACY.  The slack is part of the specification: it decides which nodes are
//      entered, not which candidate wins.
//      (A BLAS whose leaves share triangles — the reference's SBVH with spatial splits — holds such a triangle once per slot under a box that
//      covers only its part: the same triangle answers, the slot reported may be another of its slots.)
//   5. Of an inner node's two children the one with the smaller key goes first, the left one on a tie (or when only it passes).
//   6. The other child, if it passes, is pushed with its key and tested AGAIN when popped: by key <= bound while rule 3 holds (the key of a
//      passed node does not depend on the bound, so the re-test reads no memory), by rule 4 on its fetched box afterwards.
//   7. A TLAS leaf takes its instances in tlas_indices order, stepped through in two registers, not on the stack; a BLAS leaf its slots in order.
//   STACK: a push happens only at an inner node and leaves one sibling per level of the current path: at most rtxnp::stack_need() entries.
//   The caller checks it; there is no overflow path.
//   FILTER (rtx_query_sweep_filtered): the rule and the places of rtx_nearest_math.h's FILTER — a row whose mask is 0 gets the no-answer
//   record without a walk, a hidden sphere or plane is passed over in step 2, a hidden instance in step 7 before its matrix or its BLAS is
//   touched.  Hidden objects neither stop the ball nor overlap it; ACCURACY holds against the exhaustive search over the visible primitives.
//
// ACCURACY (sweep_bound() below), stated in DISTANCE: t itself is ill-conditioned for a grazing contact (it moves by sqrt of the error),
//   the distance from c(t) is not.  u = 2^-24.  S = |co - p0| + |e1| + |e2| for a triangle, |o - c| + R for a sphere, |o| + |distance| for a
//   plane, and for a box the distance from the origin to its farthest corner; T = t * |d|, the length travelled.
//   rims    ma: u S.  fm, fd: two dot products (3u each) and a quotient; mp = ma - e * fm: a product, a difference: under 8u S for mp, 8u
//           relative for dp, which reaches the contact multiplied by t: 8u T.  approach: tc one dot product and a quotient, k = mp + dp * tc
//           with |k| <= |mp|: 8u S more.  With k and w the point c(t) lies at squared distance k.k + w * (dp.dp) from the edge's line: the roundings
//           of k.k, of the difference from r * r, of the quotient and the root are relative to r * r (|k| <= r for a contact), 3u r in
//           distance; an error of w moves t, not the distance beyond this — no term is divided by r or by the half chord.  t = tc - sq and
//           c(t) = m + cd * t: u (S + r) + 2u T along the ray.  Under 18u S + 10u T + 4u r; a vertex sphere has fewer steps.
//   face    h and g: 3u |n| (|m| + t |cd|); rn: 2u r |n|; the quotient u.  The rounded n = e1 x e2 is tilted by 3u kappa, kappa = |e1||e2| / |n|,
//           and h + tp * g = n.c(tp) sees the tilt only over the contact point's offset inside the triangle: 3u kappa (|e1| + |e2|).  For
//           kappa <= 4: under 16u S + 4u T + 3u r.  Slivers beyond that are outside this bound, as in rtx_nearest_math.h: their plane is
//           ill-conditioned along the triangle.  A contact the inside test puts off the triangle by a rounding is met by the rim there.
//   So candidate_error = 24u S + 10u T + 4u r covers the distance from c(t) to the returned primitive, against r; an overlap candidate
//   has rtx_nearest_math.h's 16u S.  What may be passed over: the plane early-out compares with a rounded 3u S + 3u T + 3u r, the box
//   tests skip no computed candidate of an instance (SLACK), and the t a candidate loses to is the t of another candidate with an error of
//   its own: a primitive passed over before the returned t was nearer than r by at most twice candidate_error.  A transformed instance adds the
//   8u W of rtx_nearest_math.h, W = |o| + |co| (0 for an identity matrix), and cd's 4u relative, 4u T: a TLAS box is
//   world space while the candidates under it are computed in local space, so there, and by ORDER, the walk's t may differ from the exhaustive one.
//     sweep_bound(S, W, T, r) = (56 S + 8 W + 24 T + 8 r) * 2^-24, S the largest of the primitives and boxes compared.
//   For the returned t: the true distance from c(t) to the returned primitive is within the bound of r (<= r + bound for an overlap), and no
//   primitive is nearer than r - bound to c(t') for any t' < t.  Every term is linear in u times a length; none needed a class of its own.
#pragma once
#include <stdint.h>
#include "rtx_hits_math.h"

namespace rtxsp {

using rtxnp::P3;
using rtxnp::mk;
using rtxnp::add;
using rtxnp::sub;
using rtxnp::scale;
using rtxnp::dot;
using rtxnp::ptr3;
using rtxnp::root;
using rtxnp::infinity;
using rtxnp::is_finite;
using rtxnp::KIND_NONE;
using rtxnp::KIND_SPHERE;
using rtxnp::KIND_PLANE;
using rtxnp::KIND_TRI;
using rtxhp::cross;
using rtxhp::min_ref;
using rtxhp::max_ref;

// the winning candidate: object = instance / sphere / plane index, slot = the triangle's slot in its BLAS, (u, v) its weights; t = the bound
struct Answer { int32_t kind, object, slot; float u, v, t, d20; };

RTX_HDF bool row_is_live(const float * r) { return rtxhp::row_is_live(r) && is_finite(r[7]) && r[7] > 0.0f; }
RTX_HDF float magnitude(float f) { return f < 0.0f ? -f : f; }

RTX_HDF bool approach(P3 m, P3 d, float q2, float & tc, float & sq) {
    const float dd = dot(d, d);
    tc = -dot(m, d) / dd;
    const P3 k = add(m, scale(d, tc));
    const float w = (q2 - dot(k, k)) / dd;
    if (!(w >= 0.0f)) return false;
    sq = root(w);
    return true;
}
RTX_HDF bool entry_time(float tc, float sq, float & t) {
    t = tc - sq;
    if (t >= 0.0f) return true;
    if (!(tc + sq >= 0.0f)) return false;
    t = 0.0f;
    return true;
}
RTX_HDF bool edge_sweep(P3 ma, P3 e, P3 cd, float r2, float & t, float & s) {
    const float ee = dot(e, e);
    const float fm = dot(ma, e) / ee, fd = dot(cd, e) / ee;
    const P3 mp = sub(ma, scale(e, fm)), dp = sub(cd, scale(e, fd));
    float tc, sq;
    if (!approach(mp, dp, r2, tc, sq) || !entry_time(tc, sq, t)) return false;
    s = fm + t * fd;
    return (s >= 0.0f) & (s <= 1.0f);
}
RTX_HDF bool vertex_sweep(P3 ma, P3 cd, float r2, float & t) {
    float tc, sq;
    return approach(ma, cd, r2, tc, sq) && entry_time(tc, sq, t);
}

// the candidate of triangle (p0, e1, e2) for the local ray (co, cd) and radius r; bound, best_d20: the (t, d20) of the walk's current answer
RTX_HDF bool triangle_sweep(P3 p0, P3 e1, P3 e2, P3 co, P3 cd, float r, float bound, float & t, float & u, float & v, float & d20, float best_d20 = infinity()) {
    const P3 m = sub(co, p0);
    const P3 n = cross(e1, e2);
    const float h = dot(n, m), g = dot(n, cd), rn = r * root(dot(n, n));
    const float ah = magnitude(h);
    float tp = 0.0f;
    if (ah > rn) {
        const float s = h > 0.0f ? -g : g;
        if (!(s > 0.0f)) return false;
        tp = (ah - rn) / s;
        if (!(tp <= bound)) return false;
    }
    const float r2 = r * r;
    d20 = rtxnp::triangle_d2(m, e1, e2, u, v);
    if (d20 <= r2) { t = 0.0f; return true; }
    if ((bound == 0.0f) & (d20 > best_d20)) return false;
    {
        const P3 c = add(m, scale(cd, tp));
        const float aa = dot(e1, e1), ab = dot(e1, e2), cc = dot(e2, e2), d1 = dot(e1, c), d2 = dot(e2, c);
        const float det = aa * cc - ab * ab;
        const float fu = (cc * d1 - ab * d2) / det, fv = (aa * d2 - ab * d1) / det;
        if ((fu >= 0.0f) & (fv >= 0.0f) & ((fu + fv) <= 1.0f)) { t = tp; u = fu; v = fv; return true; }
    }
    bool any = false;
    float tt, s;
    t = infinity();
    if (edge_sweep(m, e1, cd, r2, tt, s) && tt < t) { t = tt; u = s; v = 0.0f; any = true; }
    if (edge_sweep(m, e2, cd, r2, tt, s) && tt < t) { t = tt; u = 0.0f; v = s; any = true; }
    const P3 mb = sub(m, e1), mc = sub(m, e2);
    if (edge_sweep(mb, sub(e2, e1), cd, r2, tt, s) && tt < t) { t = tt; u = 1.0f - s; v = s; any = true; }
    if (vertex_sweep(m, cd, r2, tt) && tt < t) { t = tt; u = 0.0f; v = 0.0f; any = true; }
    if (vertex_sweep(mb, cd, r2, tt) && tt < t) { t = tt; u = 1.0f; v = 0.0f; any = true; }
    if (vertex_sweep(mc, cd, r2, tt) && tt < t) { t = tt; u = 0.0f; v = 1.0f; any = true; }
    return any;
}

RTX_HDF bool sphere_sweep(P3 center, float radius_squared, P3 o, P3 d, float r, float & t, float & d20) {
    const P3 m = sub(o, center);
    const float R = root(radius_squared), s = root(dot(m, m)) - R;
    d20 = s * s;
    if (magnitude(s) <= r) { t = 0.0f; return true; }
    float tc, sq;
    if (s > 0.0f) { const float q = R + r; return approach(m, d, q * q, tc, sq) && entry_time(tc, sq, t); }
    if (!(s < 0.0f)) return false;                                             // a NaN
    const float q = R - r, dd = dot(d, d);
    tc = -dot(m, d) / dd;
    const P3 k = add(m, scale(d, tc));
    t = max_ref(tc + root(max_ref((q * q - dot(k, k)) / dd, 0.0f)), 0.0f);
    return true;
}
RTX_HDF bool plane_sweep(P3 n, float distance, P3 o, P3 d, float r, float & t, float & d20) {
    const float s = dot(n, o) + distance;
    d20 = s * s;
    const float as = magnitude(s);
    if (as <= r) { t = 0.0f; return true; }
    const float g = dot(n, d), a = s > 0.0f ? -g : g;
    if (!(a > 0.0f)) return false;
    t = (as - r) / a;
    return true;
}

// SLACK of rules 3 and 4
RTX_HDF float slack(P3 mn, P3 mx, P3 o, float r) {
    const float sigma = max_ref(magnitude(mn.x - o.x), magnitude(mx.x - o.x)) + (max_ref(magnitude(mn.y - o.y), magnitude(mx.y - o.y)) + max_ref(magnitude(mn.z - o.z), magnitude(mx.z - o.z)));
    return (160.0f * sigma + 32.0f * r) * 5.9604644775390625e-08f;
}
// rule 3: the local ray against a box grown by g; key orders the children and is the pop-time re-test
RTX_HDF bool slab(P3 mn, P3 mx, P3 o, P3 inv, float g, float bound, float & key) {
    const P3 t0 = mk(((mn.x - g) - o.x) * inv.x, ((mn.y - g) - o.y) * inv.y, ((mn.z - g) - o.z) * inv.z);
    const P3 t1 = mk(((mx.x + g) - o.x) * inv.x, ((mx.y + g) - o.y) * inv.y, ((mx.z + g) - o.z) * inv.z);
    const P3 tmin = mk(min_ref(t0.x, t1.x), min_ref(t0.y, t1.y), min_ref(t0.z, t1.z));
    const P3 tmax = mk(max_ref(t0.x, t1.x), max_ref(t0.y, t1.y), max_ref(t0.z, t1.z));
    key = max_ref(max_ref(0.0f, tmin.x), max_ref(tmin.y, tmin.z));
    const float t_exit = min_ref(tmax.x, min_ref(tmax.y, tmax.z));
    return (key <= t_exit) & (key <= bound);
}

RTX_HDF float sweep_bound(float local_scale, float world_scale, float travelled, float radius) {
    return (56.0f * local_scale + 8.0f * world_scale + 24.0f * travelled + 8.0f * radius) * 5.9604644775390625e-08f;
}
// the centre of the ball at the contact
RTX_HDF P3 centre_at(P3 o, P3 d, float t) { return t == 0.0f ? o : rtxhp::point_at(o, d, t); }

RTX_HDF void clear(Answer & a) { a.kind = KIND_NONE; a.object = -1; a.slot = -1; a.u = 0.0f; a.v = 0.0f; a.t = infinity(); a.d20 = infinity(); }
RTX_HDF void offer(Answer & a, float D, float t, float d20, int32_t kind, int32_t object, int32_t slot, float u, float v) {
    if (!(t < D)) return;
    const bool lower = kind != a.kind ? kind < a.kind : object != a.object ? object < a.object : slot < a.slot;
    if (a.kind == KIND_NONE || t < a.t || (t == a.t && (d20 < a.d20 || (d20 == a.d20 && lower)))) { a.t = t; a.d20 = d20; a.kind = kind; a.object = object; a.slot = slot; a.u = u; a.v = v; }
}
RTX_HDF bool overlapped(const Answer & a) { return a.kind != KIND_NONE && a.t == 0.0f; }
// rules 3 and 4
RTX_HDF bool node_pass(const Answer & a, P3 mn, P3 mx, P3 o, P3 inv, float r, float & key) {
    const float e = slack(mn, mx, o, r);
    if (overlapped(a)) { const float lim = root(a.d20) + e; key = rtxnp::box_d2(o, mn, mx); return key <= lim * lim; }
    return slab(mn, mx, o, inv, r + e, a.t, key);
}

// spheres and planes of a live row: step 2 of the walk, and of the exhaustive search.  a.t holds D on entry.
template <typename Scene>
RTX_HDF void world_primitives(Scene & sc, Answer & a, const P3 o, const P3 d, const float D, const float r) {
    for (int i = 0; i < sc.sphere_count(); i++) {
        if (!sc.sphere_visible(i)) continue;
        P3 c; float r2, t, d20;
        sc.sphere(i, c, r2);
        if (sphere_sweep(c, r2, o, d, r, t, d20)) offer(a, D, t, d20, KIND_SPHERE, i, -1, 0.0f, 0.0f);
    }
    for (int i = 0; i < sc.plane_count(); i++) {
        if (!sc.plane_visible(i)) continue;
        P3 n; float dist, t, d20;
        sc.plane(i, n, dist);
        if (plane_sweep(n, dist, o, d, r, t, d20)) offer(a, D, t, d20, KIND_PLANE, i, -1, 0.0f, 0.0f);
    }
}

// The walk.  Scene gives the records as for rtxhp::walk (enter(slot, o, d, co, cd) makes the BLAS of instance tlas_indices[slot] current,
// gives the local ray, returns that instance; FILTER's predicates).  Stack gives push(sp, node, key) and pop(sp, node, key).
template <typename Scene, typename Stack>
RTX_HDF void walk(Scene & sc, Stack & st, const float * row, Answer & a) {
    clear(a);
    if (!row_is_live(row) || !sc.row_visible()) return;
    const P3 o = mk(row[0], row[1], row[2]), d = mk(row[3], row[4], row[5]);
    const float D = row[6], r = row[7];
    a.t = D;
    world_primitives(sc, a, o, d, D, r);
    if (sc.tlas_nodes() <= 0) return;
    const P3 winv = rtxhp::rcp(d);
    P3 co = o, cd = d, cinv = winv;
    int sp = 0, floor_sp = 0, cur = -1, first = 0, count = 0, tl_i = 0, tl_end = 0, inst = 0;
    bool in_blas = false;
    float key;
    { P3 mn, mx; sc.tlas_node(0, mn, mx, first, count); if (node_pass(a, mn, mx, co, cinv, r, key)) cur = 0; }
    for (;;) {
        if (cur < 0) {
            if (in_blas && sp == floor_sp) { in_blas = false; co = o; cd = d; cinv = winv; }      // this instance is done: back to world space
            if (!in_blas && tl_i < tl_end) {                                                      // the next instance of the TLAS leaf
                if (!sc.instance_visible(tl_i)) { tl_i++; continue; }                             // FILTER: hidden from this row
                inst = sc.enter(tl_i++, o, d, co, cd);
                cinv = rtxhp::rcp(cd);
                P3 mn, mx; sc.blas_node(0, mn, mx, first, count);
                in_blas = true; floor_sp = sp;
                if (node_pass(a, mn, mx, co, cinv, r, key)) cur = 0;
                continue;
            }
            if (sp == 0) break;
            int node;
            sp--; st.pop(sp, node, key);
            const bool nearest = overlapped(a);
            if (!nearest && !(key <= a.t)) continue;
            cur = node;
            P3 mn, mx;
            if (in_blas) sc.blas_node(cur, mn, mx, first, count); else sc.tlas_node(cur, mn, mx, first, count);
            if (nearest && !node_pass(a, mn, mx, co, cinv, r, key)) { cur = -1; continue; }
        }
        if ((count & 0x3fffffff) > 0) {                                                           // a leaf: (first, count) of node cur
            const int n = count & 0x3fffffff;
            if (in_blas) {
                for (int i = first; i < first + n; i++) {
                    P3 p0, e1, e2; float t, u, v, d20;
                    sc.triangle(i, p0, e1, e2);
                    if (triangle_sweep(p0, e1, e2, co, cd, r, a.t, t, u, v, d20, a.d20)) offer(a, D, t, d20, KIND_TRI, inst, i, u, v);
                }
            } else { tl_i = first; tl_end = first + n; }
            cur = -1;
            continue;
        }
        P3 lmn, lmx, rmn, rmx; int lf, lc, rf, rc;
        const int left = first;
        if (in_blas) { sc.blas_node(left, lmn, lmx, lf, lc); sc.blas_node(left + 1, rmn, rmx, rf, rc); }
        else         { sc.tlas_node(left, lmn, lmx, lf, lc); sc.tlas_node(left + 1, rmn, rmx, rf, rc); }
        float kl, kr;
        const bool pl = node_pass(a, lmn, lmx, co, cinv, r, kl), pr = node_pass(a, rmn, rmx, co, cinv, r, kr);
        const bool left_first = pl && (!pr || kl <= kr);
        if (pl && pr) { st.push(sp, left_first ? left + 1 : left, left_first ? kr : kl); sp++; }
        if (pl || pr) { cur = left_first ? left : left + 1; first = left_first ? lf : rf; count = left_first ? lc : rc; }
        else cur = -1;
    }
}

}  // namespace rtxsp
