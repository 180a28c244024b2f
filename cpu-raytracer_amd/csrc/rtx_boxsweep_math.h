// rtx_boxsweep_math.h — the arithmetic AND the walk of swept-box queries (include/rtx.h: rtx_query_sweep_box), written once and compiled twice
// like rtx_sweep_math.h and rtx_overlap_math.h, whose functions it reuses: by hipcc into k_query_sweep_box (rtx_boxsweep.h) and by the host
// compiler into rtxh_query_sweep_box / rtxh_query_sweep_box_exhaustive (host/rtx_host.cpp) and boxsweep_check.cpp.  Unfused fp32
// (-ffp-contract=off), correctly rounded '/' and sqrtf on both sides, every sum of three products in vdot's order x + (y + z);
// min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b.  So every function here returns the same bits on the CPU and on gfx950.  Plain
// C++: no HIP types.  This comment is the specification.
//
// ROW      fourteen floats: centre c (3), direction d (3), max distance D, half extents h (3), rotation quaternion (x, y, z, w).  The box of
//          rtx_overlap_math.h's ROW over (c, h, q) moves without turning, its centre along c(t) = c + t * d, d as given, t in units of |d|.
//          A row is LIVE when its first seven floats are a live row of rtx_hits_math.h (direction not (+-0, +-0, +-0), six finite
//          components, D > 0, +INFINITY included) and (c, h, q) is a live row of rtx_overlap_math.h (finite, h_k >= 0, q.q finite and > 0).
//          Zero half extents are valid: a point box is a ray.  A dead row gets the no-answer record (t +inf, ids -1, axis -1, normal 0) and
//          is not walked.
// ANSWER   the smallest t in [0, D) at which the box touches a primitive (two-sided triangles, sphere shells, two-sided planes), the
//          primitive, and the AXIS code of the contact.  Every primitive yields at most one CANDIDATE (t, axis).  t < D is strict.
// FRAME    rtxop::world_frame over (c, h, q): the bits of rtx_query_overlap for the same box.  Per instance rtxop::local_frame, the local
//          direction cd = xform_dir(world_inv, d), and w = to_box(F, cd) = (a_k . cd), the velocity in the box frame.  In the box frame
//          the box rests and everything else moves by -w per unit of t.  The caveats of rtx_overlap_math.h's FRAME hold: exact for a rigid
//          pose, a uniform scale scales the box with the instance, a sheared matrix is outside the specification.
// TRIANGLE (triangle_sweep)  First rtxop::triangle_overlaps: if true the candidate is (0, AXIS_OVERLAP).  Otherwise the continuous
//          separating-axis test over the same 13 axes in the same order (0..2 the box axes, 3 the normal, 4..6 e_i x f1, 7..9 e_i x (f2 - f1),
//          10..12 e_i x f2), each with the lo and hi of the static test, its r grown by PAD, and vL = the axis's projection of w (w.k; n . w;
//          for e_0 x f f.y * w.z - f.z * w.y and cyclically, the spelling of p):
//            PAD       r' = r + 8 u s |L|_1, u = 2^-24, s = |v0|_1 + (|f1|_1 + |f2|_1) + |h|_1, |L|_1 the sum of the axis's absolute components
//                      (1 for a box axis).  p and r of one axis carry under 4 u |L|_1 (max |v| + max h) of rounding each; without the pad two
//                      axes of (nearly) one direction whose intervals have no thickness — a point box or a flat box against a triangle at
//                      right angles to a box axis: the box axis and the normal — would have to agree to the last bit for a contact to
//                      exist.  With it every interval is at least 16 u s |L|_1 / |vL| long and their common roundings are inside it.
//            vL == 0   the axis constrains nothing when lo <= r' and hi >= -r', and ends the candidate when not;
//            else      a = (lo - r') / vL, b = (hi + r') / vL; entry = min(a, b), exit = max(a, b).
//          best = the largest entry, axis = its index, the lowest index on a tie; t_in = max(0, best); t_out = the smallest exit.  A
//          candidate iff every a and b is a number, some vL != 0, and t_in <= t_out + 32 u t_out (touching is contact; the 32 u take the
//          relative rounding of the quotients and of vL, up to |L|_1 |w| / |vL| = 8: two parallel flat intervals under a motion that grazes
//          them more steeply than that may still miss each other, a limit of this form).  Then t = t_in and the axis code is the axis:
//          t = 0 with an axis code below 13 is a triangle within PAD of touching where the sweep starts, which the static test separates.
//          A NaN anywhere yields no candidate, so the pad triangles of rtx_build_blas stay invisible.  A zero-length cross axis has
//          p = r = vL = 0 and never constrains.  The axes are run in groups — the three box axes and the normal, then each edge's three —
//          and the function leaves after a group once t_in > t_out + 32 u t_out or t_in > bound (the walk's current t): t_in only grows
//          and t_out only shrinks, so this discards only losers and the candidate's bits do not depend on the bound.
// SPHERE   (sphere_sweep; a shell, as everywhere in the family)  x = to_box(F, centre - c), the centre in the box frame, moving as
//          x - t * w.  t = 0 where rtxop::sphere_overlaps holds.  Otherwise, with dmin2 and dmax2 of rtx_overlap_math.h's SPHERE:
//          outside (dmin2 > R^2)  the first t with dmin2(t) = R^2.  Coordinate k is inside the slab |x_k| <= h_k between
//            in_k = min(a, b) and out_k = max(a, b), a = (x_k - h_k) / w_k, b = (x_k + h_k) / w_k (w_k == 0: always, or never).  The six
//            breakpoints, sorted, cut t into at most seven pieces.  On the piece that starts at breakpoint S coordinate k is before its
//            slab (S < in_k: m_k = x_k - s h_k, s = the sign of w_k, or of x_k where w_k == 0), in it (m_k = 0, its velocity 0) or behind
//            it (S >= out_k: m_k = x_k + s h_k), and dmin2(t) = |m - t * v|^2 with v the velocity of the coordinates outside.  Pieces in
//            ascending order; rtxsp::approach(m, -v, R^2) gives tc and sq; the root tc - sq counts when it lies in the piece; a root
//            below the piece's start S' = max(S, 0) counts as S' when tc + sq >= S' (the box is inside at the start: the previous piece's
//            root rounded past its end); a piece that starts beyond the bound ends the search.
//          inside (dmax2 < R^2)   the first t with dmax2(t) = R^2, the farthest corner reaching the shell.  Breakpoints z_k = x_k / w_k
//            where a coordinate changes sign, at most four pieces, m_k = x_k + s h_k with s the coordinate's sign on the piece; the root
//            is tc + sq; a piece with no root, or a root below its start, is left at its start (the corner is outside already).
// PLANE    (plane_sweep)  s = n.c + distance, r = h_0 |n.a_0| + (h_1 |n.a_1| + h_2 |n.a_2|) as rtxop::plane_overlaps.  |s| <= r: t = 0.
//          Else g = n.d, a = s > 0 ? -g : g, a candidate iff a > 0 (approaching only): t = (|s| - r) / a.
// ORDER    the smallest t < D wins.  An exact tie goes to the lowest public (object_id, triangle_id), the order of rtxop::before, ids in the
//          numberings of rtx_query_closest (instances, then spheres, then planes; triangle_id -1 for spheres and planes).  The answer
//          depends only on WHICH candidates the walk meets, never on their order.  Which it meets is settled by the tree only within the
//          slack of rule 3 and, at t = 0, within PAD: a PAD candidate (t = 0, an axis code below 13) with a lower id that lies under a node
//          rtxop::node_overlaps rejects is met only if its node was visited before the answer settled at 0, so among candidates at t = 0
//          the reported id can depend on the tree where a triangle is within PAD of touching; t does not.
// AXIS     0..12 the winning axis of a triangle; AXIS_OVERLAP (13) for a static overlap, t = 0, whatever the primitive; AXIS_SPHERE (14); AXIS_PLANE (15);
//          -1 for no answer.
// NORMAL   the unit contact normal in world space, opposing the motion; zero for t == 0 and for no answer.  Computed after the walk from
//          the winner alone.  Triangle: the winning axis L in box-frame components (e_k; f1 x f2; e_i x f), taken to world as
//          normalise(L.x A_0 + (L.y A_1 + L.z A_2)) over the row's world axes A_k and negated if normal . d > 0.  Plane: n where s > 0, else
//          -n (n as stored).  Sphere: with x(t) = x - t * w in the world frame, from outside L = -(x(t) - clamp(x(t), -h, h)), from inside
//          L_k = x_k(t) + sign(x_k(t)) h_k; normalised the same way: from the contact point on the shell towards the box.
//
// THE WALK (walk() below; part of the specification; the structure of rtxsp::walk)
//   1. a.t = D.  A candidate with t < D replaces the answer when t < a.t, or t == a.t and it is before the answer in ORDER.
//   2. Spheres ascending, planes ascending, then the TLAS from its root.
//   3. While the answer is no overlap (none yet, or t > 0) a node is entered iff slab(): the centre's local ray against the node box grown
//      per axis by g_j = E_j + slack, E = rtxop::Frame::E, the box's own AABB in that frame: t0 = ((min - g) - c) * inv,
//      t1 = ((max + g) - c) * inv, inv = 1 / cd per component, key = max(max(0, tmin.x), max(tmin.y, tmin.z)), exit = min(tmax.x,
//      min(tmax.y, tmax.z)); pass iff key <= exit and key <= a.t.  A NaN passes nothing, as in rtxsp::slab.
//   4. Once the answer has t == 0 only another candidate at t = 0 with a lower id can still win: a node is entered iff rtxop::node_overlaps
//      with rtx_overlap_math.h's ULPS (key 0).  The candidate function stays triangle_sweep, now at a bound of 0: it returns a static overlap at
//      once and leaves every other triangle after its first group of axes unless that triangle is within PAD of touching, so what is left
//      costs the static test.  (Static tests alone would lose a PAD candidate with a lower id and make the answer depend on the order.)
//      SLACK  sigma = max(|min.x - c.x|, |max.x - c.x|) + the same of y + the same of z bounds the distance from the centre to anything in
//      the node box, and 2 sigma each edge of a triangle inside it: S <= 5 sigma + |h| in MARGIN's terms, T <= sigma + |h|_1 for the
//      contact of anything in the subtree.  A computed entry on a box axis or a well-conditioned axis is the exact entry of projections
//      moved by under margin(S, W, 1) + 64 u T (ACCURACY), so the computed max over the axes is at least the exact first contact of the box
//      grown by that epsilon in every half extent (its support grows by epsilon |L|_1 >= epsilon |L|_2), whose AABB is E_j + sqrt(3)
//      epsilon.  With sqrt(3) * (192 * (5 sigma + |h|) + 64 (sigma + |h|_1)) < 1800 sigma + 450 |h|_1, the slab's own roundings (two
//      differences, an inverse, a product: 4 u (sigma + E)) and, for a TLAS box against candidates measured in a local frame, 8 u W over the
//      world magnitude |c|_1:   slack = (2048 sigma + 512 |h|_1 + 16 |c|_1) * 2^-24.
//      GUARANTEED  a subtree whose triangles exactly stay farther than the slack from the box until a.t is the only kind skipped: no
//      triangle that truly touches the box before a.t is lost.  NOT GUARANTEED  that the walk meets every candidate the exhaustive search
//      computes: an ill-conditioned cross axis (kappa beyond 2^10) can put a computed entry anywhere below the exact one, and such a
//      candidate of the exhaustive search may lie in a subtree the slab test skips.  The walk's t is therefore never below the exhaustive
//      t, and above it only within ACCURACY.  The slack decides which nodes are entered, not which candidate wins.
//      SPLIT LEAVES  (rtx_overlap_math.h)  A BLAS with spatial splits stores a triangle in several slots, each under a box that bounds only
//      its part inside that leaf.  The slab test is conservative for the stored boxes, so the triangle answers through a slot whose leaf
//      the box reaches: the slot reported may be another slot of the same triangle than the exhaustive search's lowest one, and where two
//      triangles tie exactly (they share the vertex or the edge the box meets) the one reported may be the other; t is the same.
//   5. Of an inner node's two children the one with the smaller key goes first, the left one on a tie (or when only it passes).
//   6. The other child, if it passes, is pushed with its key and tested AGAIN when popped: by key <= a.t while rule 3 holds, by rule 4 on
//      its fetched box afterwards.
//   7. A TLAS leaf takes its instances in tlas_indices order, stepped through in two registers, not on the stack; a BLAS leaf its slots in
//      order.  One frame is held: the world frame, direction and velocity are made again from the row when an instance is done (the same
//      functions of the same floats: the same bits), so `row` must stay readable during the walk.
//   STACK: a push happens only at an inner node and leaves one sibling per level of the current path: at most rtxnp::stack_need() entries.
//   The caller checks it; there is no overflow path.
//   FILTER (rtx_query_sweep_box_filtered): the rule and the places of rtx_nearest_math.h's FILTER — a row whose mask is 0 gets the no-answer
//   record without a walk, a hidden sphere or plane is passed over in step 2, a hidden instance in step 7 before its matrix is read.
//
// ACCURACY (sweep_box_bound() below), stated in DISTANCE through the normalised signed gaps of rtx_overlap_math.h's MARGIN: t itself is
//   ill-conditioned for a grazing contact.  u = 2^-24; S, W, kappa as in MARGIN, taken at the box's place at t; T = t |d|, the length
//   travelled.  On top of MARGIN's roundings of one axis evaluation: cd = xform_dir 4 u and w = to_box 49 u, relative to |d|, reach the
//   contact multiplied by t: 53 u T; vL (a dot product or a 2 x 2 form) 4 u, the two differences and the quotient 3 u, relative to the
//   entry: under 64 u T together.  A derived axis turned by 102 u kappa (MARGIN) sees the velocity turned as well: 102 u kappa T.
//   PAD moves an entry by 8 u s |L|_1 / |L|_2 <= 14 u s as a normalised gap, s <= sqrt(3) S: under 32 u S.
//     sweep_box_bound(S, W, T, kappa) = margin(S, W, kappa) + (32 S + (64 + 128 kappa) T) * 2^-24
//   For the returned t: the returned primitive's exact maximal gap over its axes, the box at c(t), lies within the bound of 0 (an overlap
//   at t = 0: it is at most the bound), and no primitive has every gap below -sweep_box_bound(S, W, T', 1) at any t' < t.  Excluded, as in
//   the siblings: axes with kappa beyond 2^10 and slivers with |e1||e2| / |e1 x e2| > 4.
// OUT OF SCOPE  contact points or manifolds, rotation during the sweep, capsules and hulls, all contacts along the path, the rtx_group_* path.
#pragma once
#include <stdint.h>
#include "rtx_sweep_math.h"
#include "rtx_overlap_math.h"

namespace rtxbs {

using rtxnp::P3;
using rtxnp::mk;
using rtxnp::add;
using rtxnp::sub;
using rtxnp::scale;
using rtxnp::dot;
using rtxnp::root;
using rtxnp::infinity;
using rtxop::Frame;
using rtxop::to_box;
using rtxop::min_ref;
using rtxop::max_ref;
using rtxop::mag;
using rtxop::cross;

enum { ROW_FLOATS = 14, KEY_FLOATS = 7 };
enum { AXIS_NONE = -1, AXIS_OVERLAP = 13, AXIS_SPHERE = 14, AXIS_PLANE = 15 };

// the winning candidate: object in the public numbering, slot = the triangle's slot in its BLAS or -1; t = the walk's bound
struct Answer { int32_t object, slot, axis; float t; };

// (c, h, q) of a row as a row of rtx_overlap_math.h
RTX_HDF void box_row(const float * r, float (&b)[rtxop::ROW_FLOATS]) {
    b[0] = r[0]; b[1] = r[1]; b[2] = r[2];
    for (int k = 0; k < 7; k++) b[3 + k] = r[7 + k];
}
RTX_HDF bool row_is_live(const float * r) {
    float b[rtxop::ROW_FLOATS];
    box_row(r, b);
    return rtxhp::row_is_live(r) && rtxop::row_is_live(b);
}
RTX_HDF Frame world_frame(const float * r) {
    float b[rtxop::ROW_FLOATS];
    box_row(r, b);
    return rtxop::world_frame(b);
}

// TRIANGLE: the running interval of the continuous separating-axis test
struct Sat { float best, t_out, pad; int axis; bool ok; };            // pad = 8 u s
RTX_HDF void sat_axis(Sat & s, const int k, const float lo, const float hi, const float r0, const float vL, const float l1) {
    const float r = r0 + s.pad * l1;
    if (vL == 0.0f) { s.ok = s.ok & rtxop::axis_passes(lo, hi, r); return; }
    const float a = (lo - r) / vL, b = (hi + r) / vL;
    s.ok = s.ok & (a == a) & (b == b);
    const float entry = min_ref(a, b), exit = max_ref(a, b);
    if (entry > s.best) { s.best = entry; s.axis = k; }
    s.t_out = min_ref(s.t_out, exit);
}
RTX_HDF bool sat_live(const Sat & s, const float bound) {
    const float t_in = max_ref(0.0f, s.best);
    return s.ok & (t_in <= s.t_out + (32.0f * rtxop::unit_roundoff()) * s.t_out) & (t_in <= bound);
}
// the three cross axes e_i x f of one edge, axes k .. k + 2: va a vertex of the edge, vb the opposite vertex (rtxop::edge_passes)
RTX_HDF void sat_edge(Sat & s, const int k, const P3 f, const P3 va, const P3 vb, const P3 h, const P3 w) {
    const float ax = mag(f.x), ay = mag(f.y), az = mag(f.z);
    const float a0 = f.y * va.z - f.z * va.y, b0 = f.y * vb.z - f.z * vb.y;
    sat_axis(s, k, min_ref(a0, b0), max_ref(a0, b0), h.y * az + h.z * ay, f.y * w.z - f.z * w.y, ay + az);
    const float a1 = f.z * va.x - f.x * va.z, b1 = f.z * vb.x - f.x * vb.z;
    sat_axis(s, k + 1, min_ref(a1, b1), max_ref(a1, b1), h.x * az + h.z * ax, f.z * w.x - f.x * w.z, ax + az);
    const float a2 = f.x * va.y - f.y * va.x, b2 = f.x * vb.y - f.y * vb.x;
    sat_axis(s, k + 2, min_ref(a2, b2), max_ref(a2, b2), h.x * ay + h.y * ax, f.x * w.y - f.y * w.x, ax + ay);
}
// the candidate of triangle (p0, e1, e2) for the box F moving by w (box frame); bound: the t of the walk's current answer
RTX_HDF bool triangle_sweep(const Frame & F, const P3 w, const P3 p0, const P3 e1, const P3 e2, const float bound, float & t, int & axis) {
    if (rtxop::triangle_overlaps(F, p0, e1, e2)) { t = 0.0f; axis = AXIS_OVERLAP; return true; }
    const P3 v0 = to_box(F, sub(p0, F.c)), f1 = to_box(F, e1), f2 = to_box(F, e2);
    const P3 v1 = add(v0, f1), v2 = add(v0, f2), h = F.h;
    const float scale1 = (rtxop::norm1(v0) + (rtxop::norm1(f1) + rtxop::norm1(f2))) + rtxop::norm1(h);
    Sat s = { -infinity(), infinity(), (8.0f * rtxop::unit_roundoff()) * scale1, -1, true };
    sat_axis(s, 0, min_ref(min_ref(v0.x, v1.x), v2.x), max_ref(max_ref(v0.x, v1.x), v2.x), h.x, w.x, 1.0f);
    sat_axis(s, 1, min_ref(min_ref(v0.y, v1.y), v2.y), max_ref(max_ref(v0.y, v1.y), v2.y), h.y, w.y, 1.0f);
    sat_axis(s, 2, min_ref(min_ref(v0.z, v1.z), v2.z), max_ref(max_ref(v0.z, v1.z), v2.z), h.z, w.z, 1.0f);
    const P3 n = cross(f1, f2);
    const float pn = dot(n, v0);
    sat_axis(s, 3, pn, pn, h.x * mag(n.x) + (h.y * mag(n.y) + h.z * mag(n.z)), dot(n, w), rtxop::norm1(n));
    if (!sat_live(s, bound)) return false;
    sat_edge(s, 4, f1, v0, v2, h, w);
    if (!sat_live(s, bound)) return false;
    sat_edge(s, 7, sub(f2, f1), v1, v0, h, w);
    if (!sat_live(s, bound)) return false;
    sat_edge(s, 10, f2, v0, v1, h, w);
    if (!sat_live(s, bound) || s.axis < 0) return false;
    t = max_ref(0.0f, s.best); axis = s.axis;
    return true;
}

RTX_HDF void order2(float & a, float & b) { const float lo = min_ref(a, b), hi = max_ref(a, b); a = lo; b = hi; }
RTX_HDF float sign_of(float v, float fallback) { return v > 0.0f ? 1.0f : v < 0.0f ? -1.0f : fallback < 0.0f ? -1.0f : 1.0f; }
// SPHERE
RTX_HDF bool sphere_sweep(const Frame & F, const P3 w, const P3 center, const float R2, const float bound, float & t) {
    if (rtxop::sphere_overlaps(F, center, R2)) { t = 0.0f; return true; }
    if (!(dot(w, w) > 0.0f)) return false;
    const P3 x = to_box(F, sub(center, F.c)), h = F.h;
    const float xs[3] = { x.x, x.y, x.z }, hs[3] = { h.x, h.y, h.z }, ws[3] = { w.x, w.y, w.z };
    const float nx = max_ref(mag(x.x) - h.x, 0.0f), ny = max_ref(mag(x.y) - h.y, 0.0f), nz = max_ref(mag(x.z) - h.z, 0.0f);
    float sg[3];
    for (int k = 0; k < 3; k++) sg[k] = sign_of(ws[k], xs[k]);
    if (nx * nx + (ny * ny + nz * nz) > R2) {                                   // outside: dmin2(t) = R^2
        float in[3], out[3];
        for (int k = 0; k < 3; k++) {
            if (ws[k] == 0.0f) { const bool inside = mag(xs[k]) <= hs[k]; in[k] = inside ? -infinity() : infinity(); out[k] = infinity(); }
            else { const float a = (xs[k] - hs[k]) / ws[k], b = (xs[k] + hs[k]) / ws[k]; in[k] = min_ref(a, b); out[k] = max_ref(a, b); }
        }
        float T[6] = { in[0], out[0], in[1], out[1], in[2], out[2] };
        order2(T[0], T[5]); order2(T[1], T[3]); order2(T[2], T[4]);
        order2(T[1], T[2]); order2(T[3], T[4]);
        order2(T[0], T[3]); order2(T[2], T[5]);
        order2(T[0], T[1]); order2(T[2], T[3]); order2(T[4], T[5]);
        order2(T[1], T[2]); order2(T[3], T[4]);
        for (int j = 0; j < 7; j++) {
            const float S = j == 0 ? -infinity() : T[j - 1], E = j == 6 ? infinity() : T[j];
            if (E < 0.0f) continue;
            const float S0 = max_ref(S, 0.0f);
            if (S0 > bound) return false;
            float m[3], v[3];
            for (int k = 0; k < 3; k++) {
                const bool behind = S >= out[k], within = !behind & (S >= in[k]);
                m[k] = within ? 0.0f : behind ? xs[k] + sg[k] * hs[k] : xs[k] - sg[k] * hs[k];
                v[k] = within ? 0.0f : -ws[k];
            }
            float tc, sq;
            if (!rtxsp::approach(mk(m[0], m[1], m[2]), mk(v[0], v[1], v[2]), R2, tc, sq)) continue;
            const float tr = tc - sq;
            if (tr < S0) { if (tc + sq >= S0) { t = S0; return true; } continue; }
            if (tr <= E) { t = tr; return true; }
        }
        return false;
    }
    float z[3];                                                                 // inside: dmax2(t) = R^2
    for (int k = 0; k < 3; k++) z[k] = ws[k] == 0.0f ? infinity() : xs[k] / ws[k];
    float Z[3] = { z[0], z[1], z[2] };
    order2(Z[0], Z[1]); order2(Z[1], Z[2]); order2(Z[0], Z[1]);
    for (int j = 0; j < 4; j++) {
        const float S = j == 0 ? -infinity() : Z[j - 1], E = j == 3 ? infinity() : Z[j];
        if (E < 0.0f) continue;
        const float S0 = max_ref(S, 0.0f);
        if (S0 > bound) return false;
        float m[3];
        for (int k = 0; k < 3; k++) m[k] = S >= z[k] ? xs[k] - sg[k] * hs[k] : xs[k] + sg[k] * hs[k];
        float tc, sq;
        if (!rtxsp::approach(mk(m[0], m[1], m[2]), mk(-w.x, -w.y, -w.z), R2, tc, sq)) { t = S0; return true; }
        const float tr = tc + sq;
        if (tr < S0) { t = S0; return true; }
        if (tr <= E) { t = tr; return true; }
    }
    return false;
}
// PLANE: F and d in world space
RTX_HDF bool plane_sweep(const Frame & F, const P3 d, const P3 n, const float distance, float & t) {
    const float s = dot(n, F.c) + distance;
    const float r = F.h.x * mag(dot(n, F.a0)) + (F.h.y * mag(dot(n, F.a1)) + F.h.z * mag(dot(n, F.a2)));
    const float as = mag(s);
    if (as <= r) { t = 0.0f; return true; }
    const float g = dot(n, d), a = s > 0.0f ? -g : g;
    if (!(a > 0.0f)) return false;
    t = (as - r) / a;
    return true;
}

// NORMAL
RTX_HDF P3 world_normal(const Frame & W, const P3 L) {
    const P3 n = mk(L.x * W.a0.x + (L.y * W.a1.x + L.z * W.a2.x), L.x * W.a0.y + (L.y * W.a1.y + L.z * W.a2.y), L.x * W.a0.z + (L.y * W.a1.z + L.z * W.a2.z));
    const float l = root(dot(n, n));
    if (!(l > 0.0f)) return mk(0.0f, 0.0f, 0.0f);
    return mk(n.x / l, n.y / l, n.z / l);
}
// W: the row's world frame; world_inv, e1, e2: the winner's instance and hot record; axis in 0..12
RTX_HDF P3 triangle_normal(const Frame & W, const float * world_inv, const P3 e1, const P3 e2, const int axis, const P3 d) {
    const Frame F = rtxop::local_frame(W, world_inv);
    const P3 f1 = to_box(F, e1), f2 = to_box(F, e2);
    P3 L;
    if (axis < 3) L = mk(axis == 0 ? 1.0f : 0.0f, axis == 1 ? 1.0f : 0.0f, axis == 2 ? 1.0f : 0.0f);
    else if (axis == 3) L = cross(f1, f2);
    else {
        const int e = (axis - 4) / 3, i = (axis - 4) % 3;
        const P3 f = e == 0 ? f1 : e == 1 ? sub(f2, f1) : f2;
        L = i == 0 ? mk(0.0f, -f.z, f.y) : i == 1 ? mk(f.z, 0.0f, -f.x) : mk(-f.y, f.x, 0.0f);
    }
    const P3 n = world_normal(W, L);
    return dot(n, d) > 0.0f ? mk(-n.x, -n.y, -n.z) : n;
}
RTX_HDF P3 sphere_normal(const Frame & W, const P3 d, const P3 center, const float R2, const float t) {
    const P3 x0 = to_box(W, sub(center, W.c)), w = to_box(W, d), h = W.h;
    const float nx = max_ref(mag(x0.x) - h.x, 0.0f), ny = max_ref(mag(x0.y) - h.y, 0.0f), nz = max_ref(mag(x0.z) - h.z, 0.0f);
    const bool outside = nx * nx + (ny * ny + nz * nz) > R2;
    const P3 x = sub(x0, scale(w, t));
    P3 L;
    if (outside) L = mk(-(x.x - max_ref(-h.x, min_ref(x.x, h.x))), -(x.y - max_ref(-h.y, min_ref(x.y, h.y))), -(x.z - max_ref(-h.z, min_ref(x.z, h.z))));
    else L = mk(x.x + sign_of(x.x, 1.0f) * h.x, x.y + sign_of(x.y, 1.0f) * h.y, x.z + sign_of(x.z, 1.0f) * h.z);
    return world_normal(W, L);
}
RTX_HDF P3 plane_normal(const Frame & W, const P3 n, const float distance) {
    return dot(n, W.c) + distance > 0.0f ? n : mk(-n.x, -n.y, -n.z);
}

RTX_HDF float sweep_box_bound(float local_scale, float world_scale, float travelled, float kappa) {
    return rtxop::margin(local_scale, world_scale, kappa) + (32.0f * local_scale + (64.0f + 128.0f * kappa) * travelled) * rtxop::unit_roundoff();
}

RTX_HDF void clear(Answer & a) { a.object = -1; a.slot = -1; a.axis = AXIS_NONE; a.t = infinity(); }
RTX_HDF void offer(Answer & a, const float D, const float t, const int32_t object, const int32_t slot, const int32_t axis) {
    if (!(t < D)) return;
    if (t < a.t || (t == a.t && rtxop::before(object, slot, a.object, a.slot))) { a.t = t; a.object = object; a.slot = slot; a.axis = axis; }
}
RTX_HDF bool overlapped(const Answer & a) { return a.object >= 0 && a.t == 0.0f; }
RTX_HDF void finish(Answer & a) { if (a.object < 0) a.t = infinity(); }

// SLACK of rule 3
RTX_HDF float slack(const P3 mn, const P3 mx, const Frame & F) {
    const P3 o = F.c;
    const float sigma = max_ref(mag(mn.x - o.x), mag(mx.x - o.x)) + (max_ref(mag(mn.y - o.y), mag(mx.y - o.y)) + max_ref(mag(mn.z - o.z), mag(mx.z - o.z)));
    return (2048.0f * sigma + 512.0f * rtxop::norm1(F.h) + 16.0f * rtxop::norm1(o)) * rtxop::unit_roundoff();
}
// rule 3: rtxsp::slab with a growth per axis
RTX_HDF bool slab(const P3 mn, const P3 mx, const P3 o, const P3 inv, const P3 g, const float bound, float & key) {
    const P3 t0 = mk(((mn.x - g.x) - o.x) * inv.x, ((mn.y - g.y) - o.y) * inv.y, ((mn.z - g.z) - o.z) * inv.z);
    const P3 t1 = mk(((mx.x + g.x) - o.x) * inv.x, ((mx.y + g.y) - o.y) * inv.y, ((mx.z + g.z) - o.z) * inv.z);
    const P3 tmin = mk(min_ref(t0.x, t1.x), min_ref(t0.y, t1.y), min_ref(t0.z, t1.z));
    const P3 tmax = mk(max_ref(t0.x, t1.x), max_ref(t0.y, t1.y), max_ref(t0.z, t1.z));
    key = max_ref(max_ref(0.0f, tmin.x), max_ref(tmin.y, tmin.z));
    const float t_exit = min_ref(tmax.x, min_ref(tmax.y, tmax.z));
    return (key <= t_exit) & (key <= bound);
}
// rules 3 and 4
RTX_HDF bool node_pass(const Answer & a, const Frame & F, const P3 mn, const P3 mx, const P3 inv, const float ulps, float & key) {
    if (overlapped(a)) { key = 0.0f; return rtxop::node_overlaps(F, mn, mx, ulps); }
    const float e = slack(mn, mx, F);
    return slab(mn, mx, F.c, inv, mk(F.E.x + e, F.E.y + e, F.E.z + e), a.t, key);
}

// spheres and planes of a live row: step 2 of the walk, and of the exhaustive search.  a.t holds D on entry; W, d, w in world space
template <typename Scene>
RTX_HDF void world_primitives(Scene & sc, Answer & a, const Frame & W, const P3 d, const P3 w, const float D) {
    const int32_t ic = sc.instance_count(), sn = sc.sphere_count();
    for (int i = 0; i < sn; i++) {
        if (!sc.sphere_visible(i)) continue;
        P3 c; float r2, t;
        sc.sphere(i, c, r2);
        if (sphere_sweep(W, w, c, r2, a.t, t)) offer(a, D, t, ic + i, -1, t == 0.0f ? (int)AXIS_OVERLAP : (int)AXIS_SPHERE);
    }
    for (int i = 0; i < sc.plane_count(); i++) {
        if (!sc.plane_visible(i)) continue;
        P3 n; float dist, t;
        sc.plane(i, n, dist);
        if (plane_sweep(W, d, n, dist, t)) offer(a, D, t, ic + sn + i, -1, t == 0.0f ? (int)AXIS_OVERLAP : (int)AXIS_PLANE);
    }
}

// The walk.  Scene gives the records as for rtxop::walk; enter(slot, F, cd) makes the BLAS of instance tlas_indices[slot] current, turns the
// world frame F and the world direction cd into that instance's local ones and returns that instance.  Stack gives push(sp, node, key) and
// pop(sp, node, key).
template <typename Scene, typename Stack>
RTX_HDF void walk(Scene & sc, Stack & st, const float * row, Answer & a) {
    clear(a);
    if (!row_is_live(row) || !sc.row_visible()) return;
    const float D = row[6];
    a.t = D;
    Frame F = world_frame(row);
    P3 cd = mk(row[3], row[4], row[5]);
    P3 w = to_box(F, cd);
    world_primitives(sc, a, F, cd, w, D);
    if (sc.tlas_nodes() <= 0) { finish(a); return; }
    P3 cinv = rtxhp::rcp(cd);
    int sp = 0, floor_sp = 0, cur = -1, first = 0, count = 0, tl_i = 0, tl_end = 0, inst = 0;
    bool in_blas = false;
    float key;
    { P3 mn, mx; sc.tlas_node(0, mn, mx, first, count); if (node_pass(a, F, mn, mx, cinv, (float)rtxop::TLAS_ULPS, key)) cur = 0; }
    for (;;) {
        if (cur < 0) {
            if (in_blas && sp == floor_sp) {                                                      // this instance is done: back to world space
                in_blas = false;
                F = world_frame(row); cd = mk(row[3], row[4], row[5]); w = to_box(F, cd); cinv = rtxhp::rcp(cd);
            }
            if (!in_blas && tl_i < tl_end) {                                                      // the next instance of the TLAS leaf
                if (!sc.instance_visible(tl_i)) { tl_i++; continue; }                             // FILTER: hidden from this row
                inst = sc.enter(tl_i++, F, cd);
                w = to_box(F, cd); cinv = rtxhp::rcp(cd);
                P3 mn, mx; sc.blas_node(0, mn, mx, first, count);
                in_blas = true; floor_sp = sp;
                if (node_pass(a, F, mn, mx, cinv, (float)rtxop::BLAS_ULPS, key)) cur = 0;
                continue;
            }
            if (sp == 0) break;
            int node;
            sp--; st.pop(sp, node, key);
            const bool settled = overlapped(a);
            if (!settled && !(key <= a.t)) continue;
            cur = node;
            P3 mn, mx;
            if (in_blas) sc.blas_node(cur, mn, mx, first, count); else sc.tlas_node(cur, mn, mx, first, count);
            if (settled && !node_pass(a, F, mn, mx, cinv, in_blas ? (float)rtxop::BLAS_ULPS : (float)rtxop::TLAS_ULPS, key)) { cur = -1; continue; }
        }
        if ((count & 0x3fffffff) > 0) {                                                           // a leaf: (first, count) of node cur
            const int n = count & 0x3fffffff;
            if (in_blas) {
                for (int i = first; i < first + n; i++) {
                    P3 p0, e1, e2; float t; int axis;
                    sc.triangle(i, p0, e1, e2);
                    if (triangle_sweep(F, w, p0, e1, e2, a.t, t, axis)) offer(a, D, t, inst, i, axis);
                }
            } else { tl_i = first; tl_end = first + n; }
            cur = -1;
            continue;
        }
        P3 lmn, lmx, rmn, rmx; int lf, lc, rf, rc;
        const int left = first;
        if (in_blas) { sc.blas_node(left, lmn, lmx, lf, lc); sc.blas_node(left + 1, rmn, rmx, rf, rc); }
        else         { sc.tlas_node(left, lmn, lmx, lf, lc); sc.tlas_node(left + 1, rmn, rmx, rf, rc); }
        const float ulps = in_blas ? (float)rtxop::BLAS_ULPS : (float)rtxop::TLAS_ULPS;
        float kl, kr;
        const bool pl = node_pass(a, F, lmn, lmx, cinv, ulps, kl), pr = node_pass(a, F, rmn, rmx, cinv, ulps, kr);
        const bool left_first = pl && (!pr || kl <= kr);
        if (pl && pr) { st.push(sp, left_first ? left + 1 : left, left_first ? kr : kl); sp++; }
        if (pl || pr) { cur = left_first ? left : left + 1; first = left_first ? lf : rf; count = left_first ? lc : rc; }
        else cur = -1;
    }
    finish(a);
}

}  // namespace rtxbs
