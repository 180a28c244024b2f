// rtx_nearest_math.h — the arithmetic AND the walk of nearest-surface-point queries (include/rtx.h: rtx_query_nearest), written once and
// compiled twice like rtx_normals_math.h: by hipcc into k_query_nearest (rtx_nearest.h) and by the host compiler into rtxh_query_nearest /
// rtxh_query_nearest_exhaustive (host/rtx_host.cpp) and nearest_check.cpp.  Unfused fp32 (-ffp-contract=off), correctly rounded '/' and
// sqrtf on both sides, every sum of three products in vdot's order x + (y + z); the transcendental functions of the sphere's uv are those of
// rtx_libm.h.  So every function here returns the same bits on the CPU and on gfx950.  Plain C++: no HIP types.  This comment is the
// specification.
//
// ROW      (x, y, z, rmax).  A row is LIVE when x, y, z are finite and rmax > 0 (a NaN rmax is not; +INFINITY is).  A dead row gets the
//          no-answer record and is not walked.
// BOX      d = max(max(min - p, p - max), 0) per axis (max(a, b) = a > b ? a : b), d2 = dx*dx + (dy*dy + dz*dz).
// TRIANGLE (p0, e1, e2) of the hot record, ap = p - p0.  The Voronoi-region closest point of Ericson, Real-Time Collision Detection 5.1.5,
//          with its six dot products taken from five: d1 = e1.ap, d2 = e2.ap, and the Gram terms aa = e1.e1, ab = e1.e2, cc = e2.e2 give
//          d3 = d1 - aa, d4 = d2 - ab, d5 = d1 - ab, d6 = d2 - cc (what e1.bp, e2.bp, e1.cp, e2.cp are in exact arithmetic; the Gram terms carry
//          a relative error, not one that grows with |ap|).  Regions in Ericson's order, the first that applies:
//            vertex a   d1 <= 0 and d2 <= 0                                   u = 0, v = 0
//            vertex b   d3 >= 0 and d4 <= d3                                  u = 1, v = 0
//            edge ab    vc = d1*d4 - d3*d2 <= 0, d1 >= 0, d3 <= 0             u = d1 / (d1 - d3), v = 0
//            vertex c   d6 >= 0 and d5 <= d6                                  u = 0, v = 1
//            edge ac    vb = d5*d2 - d1*d6 <= 0, d2 >= 0, d6 <= 0             u = 0, v = d2 / (d2 - d6)
//            edge bc    va = d3*d6 - d5*d4 <= 0, d4 - d3 >= 0, d5 - d6 >= 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), u = 1 - w, v = w
//            face       otherwise                                             k = 1 / (va + (vb + vc)), u = vb * k, v = vc * k
//          The offset from p0 is w = e1*u + e2*v, the distance vector r = ap - w, d2 = r.r, the point q = p0 + w.  d2 is taken from ap and
//          w, never from p - q: its roundings are then relative to |ap| + |e1| + |e2| and not to the size of the coordinates.  A NaN d2
//          never answers (every comparison with it is false): a degenerate triangle whose face region divides 0 by 0, a NaN vertex, the
//          pad triangles of rtx_build_blas.
// SPHERE   v = p - c, l = sqrtf(v.v), r = sqrtf(radius_squared), s = l - r, d2 = s*s.  dir = v / l per component, (0, 1, 0) when l == 0;
//          point = c + dir * r, normal = dir, uv from the normal by the formulas of rebuild_sphere_hit (rtx_shade.h).
// PLANE    s = n.p + distance, d2 = s*s, point = p - n*s, normal = n, uv = (point.u_axis, point.v_axis) as rebuild_plane_hit.
// TRIANGLE OUTPUTS  position = xform_pos(world, q); normal = xform_dir(world, vnormalize(n0 + ne1*u + ne2*v)); uv = (t0 + u*te1) + v*te2:
//          the spellings of rebuild_triangle_hit (rtx_shade.h) at the weights (u, v).
//
// THE WALK (walk() below; part of the specification, so that equal distances resolve the same way everywhere)
//   1. b2 = rmax * rmax.
//   2. A candidate with d2 < b2 (strictly) replaces the answer and lowers b2.
//   3. Candidates: spheres ascending, planes ascending, then the TLAS from its root.
//   4. A node is entered iff its box d2 < b2 (roots included).
//   5. Of an inner node's two children the one with the smaller box d2 goes first, the left one when dl <= dr.
//   6. The other child is pushed WITH its d2 if that is < b2 ...
//   7. ... and tested again against the then-current b2 when popped.
//   8. A TLAS leaf takes its instances in tlas_indices order: p_l = xform_pos(world_inv, p), the BLAS from its root with p_l and the same b2.
//      The instances of a leaf are stepped through in two registers, not on the stack.  The same b2: a world-space box distance (steps 4 .. 7
//      over the TLAS) and local distances are compared with one bound, which is right for rigid poses only — the host refuses a frame
//      with any other instance before this walk runs (rtxu::instance_rigid, rtx_update_math.h; include/rtx.h, rtx_query_nearest: Limits).
//   9. A BLAS leaf tests its slots in order.
//   FILTER (rtx_query_nearest_filtered; the same rule in rtx_hits_math.h and rtx_sweep_math.h).  Objects are numbered as RTX_AOV_OBJECT_ID
//   numbers them: instance i -> i, sphere s -> I + s, plane p -> I + S + p.  An object EXISTS for a row iff (object_mask & row_mask) != 0;
//   without a table every object_mask is 0xFFFFFFFF.  The Scene answers sphere_visible(i), plane_visible(i), instance_visible(slot) and
//   row_visible() (the row's mask is not 0); an unfiltered Scene answers true at compile time and the walk is the code it was.  A row that is
//   not visible is answered like a dead row, without a walk.  A hidden sphere or plane is not offered in step 3.  A hidden instance is passed
//   over in step 8, where the walk takes it from its TLAS leaf and before its matrix or its BLAS is touched: the leaf's next instance, if
//   any, is taken by the same loop.  Nothing else changes: TLAS boxes still contain hidden instances, and the order, the tie rules, the
//   stack rule and stack_need() are the same.  ACCURACY then holds against the exhaustive search over the visible primitives.
//   The first of several exact ties therefore wins.  STACK: a push happens only at an inner node and leaves one sibling per level of the
//   current path, so at most (TLAS inner depth + 1) + (BLAS inner depth + 1) entries are ever held (inner depth: the depth of the deepest inner
//   node, root 0, -1 for a tree that is one leaf): stack_need().  The caller checks it before a walk; there is no overflow path.
//
// ACCURACY (distance_bound() below).  u = 2^-24.  Local scale S = |ap| + |e1| + |e2|.  Roundings on a triangle candidate's path, as distances:
//   ap: u |ap|;  d1, d2: 3u |e||ap| each, the Gram terms 3u relative, so an edge or face weight moves the point by at most 4u S along the
//   triangle;  w = e1*u + e2*v: 3u (|e1| + |e2|) per component, r = ap - w one more u |r|: sqrt(3) * 4u S for the vector;  r.r: 3u relative
//   = 1.5u of the distance, sqrtf: u.  Together under 14u S; a point the region tests put on the wrong side of a region border is within
//   the same 4u S of the right one.  (The weights of a sliver, |e1||e2| / |e1 x e2| beyond 2^10, are ill-conditioned along the triangle; the
//   distance changes by that error only to second order above the face, and such slivers are outside this bound.)
//   candidate_error = 16u S: a candidate's computed distance is within 16u S of the true distance from p_l to its triangle.
//   Pruning compares a computed box d2 with b2: the box distance has one rounding per axis, three squares and two sums, under 2.5u of
//   itself, and is <= S for any triangle inside.  A subtree is skipped only when its computed box d2 >= b2, so every triangle in it has a
//   TRUE distance above b (1 - 2.5u) and a computed one above b (1 - 2.5u) - 16u S.  Hence, b the walk's distance:
//     walk >= exhaustive always (minima of one function over a subset and over the whole set);
//     walk <= exhaustive + 18.5u S, S of the exhaustive winner;
//     |walk - true minimum| <= 18.5u S, and the TRUE distance of the primitive the walk returns <= true minimum + 2 * 16u S + 2.5u S.
//   TLAS boxes are world space while an instance's candidates are measured at p_l: xform_pos rounds four times relative to |p| + |p_l|, the
//   instance box the host derived likewise, so a transformed instance adds 8u W, W = |p| + |p_l|.  An identity matrix is exact: W = 0.
//   distance_bound(S, W) = (36 S + 8 W) * 2^-24 covers all three statements (S: the larger of the primitives compared).  Spheres and planes
//   are never pruned: the walk and the exhaustive search agree on them exactly.
#pragma once
#include <stdint.h>
#include "rtx_libm.h"

#if !defined(RTX_HD)
#if defined(__HIPCC__)
#define RTX_HD __host__ __device__ inline
#else
#define RTX_HD inline
#endif
#endif
#define RTX_HDF RTX_HD __attribute__((always_inline))

namespace rtxnp {

struct P3 { float x, y, z; };
enum { KIND_NONE = 0, KIND_SPHERE = 1, KIND_PLANE = 2, KIND_TRI = 3 };      // in candidate order
// the winning candidate: object = instance / sphere / plane index, slot = the triangle's slot in its BLAS, (u, v) its weights; d2 = b2
struct Answer { int32_t kind, object, slot; float u, v, d2; };

RTX_HDF P3 mk(float x, float y, float z) { P3 r; r.x = x; r.y = y; r.z = z; return r; }
RTX_HDF P3 ptr3(const float * p) { return mk(p[0], p[1], p[2]); }
RTX_HDF P3 add(P3 a, P3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
RTX_HDF P3 sub(P3 a, P3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
RTX_HDF P3 scale(P3 a, float f) { return mk(a.x * f, a.y * f, a.z * f); }
RTX_HDF float dot(P3 l, P3 r) { return l.x * r.x + (l.y * r.y + l.z * r.z); }
RTX_HDF float max_ref(float a, float b) { return a > b ? a : b; }
RTX_HDF uint32_t float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RTX_HDF bool is_finite(float f) { return (float_bits(f) & 0x7f800000u) != 0x7f800000u; }
RTX_HDF float root(float x) { return RTX_SQRTF(x); }
RTX_HDF float infinity() { return __builtin_inff(); }
// Matrix4::transform_position / transform_direction in the order of rtx_math.h's xform_pos / xform_dir; cells[i + 4j]
RTX_HDF P3 xform_pos(const float * c, P3 d) {
    return mk(c[0] * d.x + (c[1] * d.y + (c[2]  * d.z + c[3])),
              c[4] * d.x + (c[5] * d.y + (c[6]  * d.z + c[7])),
              c[8] * d.x + (c[9] * d.y + (c[10] * d.z + c[11])));
}
RTX_HDF P3 xform_dir(const float * c, P3 d) {
    return mk(c[0] * d.x + (c[1] * d.y + c[2]  * d.z),
              c[4] * d.x + (c[5] * d.y + c[6]  * d.z),
              c[8] * d.x + (c[9] * d.y + c[10] * d.z));
}

RTX_HDF bool row_is_live(const float * r) { return is_finite(r[0]) && is_finite(r[1]) && is_finite(r[2]) && r[3] > 0.0f; }

RTX_HDF float box_d2(P3 p, P3 mn, P3 mx) {
    const float dx = max_ref(max_ref(mn.x - p.x, p.x - mx.x), 0.0f);
    const float dy = max_ref(max_ref(mn.y - p.y, p.y - mx.y), 0.0f);
    const float dz = max_ref(max_ref(mn.z - p.z, p.z - mx.z), 0.0f);
    return dx * dx + (dy * dy + dz * dz);
}

// The region chain of TRIANGLE, in its one place: the weights (u, v) of the closest point of triangle (p0, e1, e2) to p0 + ap, and the branch
// that gave them — REGION_VERTEX_A .. REGION_FACE, the feature of the triangle that holds the point (rtx_side_math.h reads it; triangle_d2
// below drops it, and its code is what it was).
enum { REGION_VERTEX_A = 0, REGION_VERTEX_B = 1, REGION_VERTEX_C = 2, REGION_EDGE_AB = 3, REGION_EDGE_BC = 4, REGION_EDGE_AC = 5, REGION_FACE = 6 };
RTX_HDF int triangle_weights(P3 ap, P3 e1, P3 e2, float & u, float & v) {
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const float aa = dot(e1, e1), ab = dot(e1, e2), cc = dot(e2, e2);
    const float d3 = d1 - aa, d4 = d2 - ab, d5 = d1 - ab, d6 = d2 - cc;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; return REGION_VERTEX_A; }
    else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; return REGION_VERTEX_B; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; return REGION_EDGE_AB; }
    else if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; return REGION_VERTEX_C; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); return REGION_EDGE_AC; }
    else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) { const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); u = 1.0f - w; v = w; return REGION_EDGE_BC; }
    else { const float k = 1.0f / (va + (vb + vc)); u = vb * k; v = vc * k; return REGION_FACE; }
}
// the weights (u, v) of the closest point of triangle (p0, e1, e2) to p0 + ap, and its squared distance
RTX_HDF float triangle_d2(P3 ap, P3 e1, P3 e2, float & u, float & v) {
    triangle_weights(ap, e1, e2, u, v);
    const P3 w = add(scale(e1, u), scale(e2, v));
    const P3 r = sub(ap, w);
    return dot(r, r);
}
RTX_HDF P3 triangle_point(P3 p0, P3 e1, P3 e2, float u, float v) { return add(p0, add(scale(e1, u), scale(e2, v))); }

RTX_HDF float sphere_d2(P3 p, P3 c, float radius_squared) {
    const P3 v = sub(p, c);
    const float s = root(dot(v, v)) - root(radius_squared);
    return s * s;
}
RTX_HDF void sphere_outputs(P3 p, P3 c, float radius_squared, P3 & point, P3 & normal, float & tu, float & tv) {
    const float ONE_OVER_PI = 0.31830988618f, ONE_OVER_TWO_PI = 0.15915494309f;
    const P3 v = sub(p, c);
    const float l = root(dot(v, v)), r = root(radius_squared);
    normal = l == 0.0f ? mk(0.0f, 1.0f, 0.0f) : mk(v.x / l, v.y / l, v.z / l);
    point = add(c, scale(normal, r));
    tu = rtx_atan2f(normal.z, normal.x) * ONE_OVER_TWO_PI + 0.5f;
    tv = rtx_acosf(normal.y) * ONE_OVER_PI + 0.5f;
}
RTX_HDF float plane_d2(P3 p, P3 n, float distance) { const float s = dot(n, p) + distance; return s * s; }
RTX_HDF void plane_outputs(P3 p, P3 n, float distance, P3 u_axis, P3 v_axis, P3 & point, P3 & normal, float & tu, float & tv) {
    const float s = dot(n, p) + distance;
    point = sub(p, scale(n, s));
    normal = n;
    tu = dot(point, u_axis); tv = dot(point, v_axis);
}
// normal and uv of a triangle answer from its cold record's fields, as rebuild_triangle_hit spells them
RTX_HDF void triangle_outputs(const float * world, P3 n0, P3 ne1, P3 ne2, const float * t0, const float * te1, const float * te2, float u, float v,
                              P3 & normal, float & tu, float & tv) {
    const P3 n = add(add(n0, scale(ne1, u)), scale(ne2, v));
    const float inv = 1.0f / root(dot(n, n));
    normal = xform_dir(world, scale(n, inv));
    tu = (t0[0] + u * te1[0]) + v * te2[0];
    tv = (t0[1] + u * te1[1]) + v * te2[1];
}

// stack entries the walk can hold at once, from the trees' inner depths (-1: the tree is one leaf)
RTX_HDF int stack_need(int tlas_inner_depth, int blas_inner_depth) { return (tlas_inner_depth + 1) + (blas_inner_depth + 1); }
// how far the walk's distance may lie above the exhaustive minimum (see ACCURACY above): local scale S, world scale W (0: identity instance)
RTX_HDF float distance_bound(float local_scale, float world_scale) { return (36.0f * local_scale + 8.0f * world_scale) * 5.9604644775390625e-08f; }

RTX_HDF void offer(Answer & a, float d2, int32_t kind, int32_t object, int32_t slot, float u, float v) {
    if (d2 < a.d2) { a.d2 = d2; a.kind = kind; a.object = object; a.slot = slot; a.u = u; a.v = v; }
}

// The walk.  Scene gives the records: sphere_count(), sphere(i, c, r2), plane_count(), plane(i, n, dist), tlas_nodes() (count, 0 = none),
// tlas_node(i, mn, mx, first, count), enter(slot, p, p_l) (makes the BLAS of instance tlas_indices[slot] current, returns that instance),
// blas_node(i, mn, mx, first, count), triangle(i, p0, e1, e2); count's low 30 bits > 0 = a leaf, children of an inner node at first, first + 1;
// and FILTER's predicates row_visible(), sphere_visible(i), plane_visible(i), instance_visible(slot) (RTX_WALK_UNFILTERED below: all true).
// Stack gives push(sp, node, d2) and pop(sp, node, d2) for entry sp.
// FILTER's predicates of a Scene that hides nothing, for the body of its struct: constants, so that the tests on them leave no code behind
#define RTX_WALK_UNFILTERED \
    static constexpr bool row_visible() { return true; } \
    static constexpr bool sphere_visible(int) { return true; } \
    static constexpr bool plane_visible(int) { return true; } \
    static constexpr bool instance_visible(int) { return true; }
// FILTER's rule
RTX_HDF bool mask_visible(uint32_t object_mask, uint32_t row_mask) { return (object_mask & row_mask) != 0u; }

template <typename Scene, typename Stack>
RTX_HDF void walk(Scene & sc, Stack & st, const float * row, Answer & a) {
    a.kind = KIND_NONE; a.object = -1; a.slot = -1; a.u = 0.0f; a.v = 0.0f; a.d2 = infinity();
    if (!row_is_live(row) || !sc.row_visible()) return;
    const P3 p = mk(row[0], row[1], row[2]);
    P3 pl = p;
    a.d2 = row[3] * row[3];
    for (int i = 0; i < sc.sphere_count(); i++) { if (!sc.sphere_visible(i)) continue; P3 c; float r2; sc.sphere(i, c, r2); offer(a, sphere_d2(p, c, r2), KIND_SPHERE, i, -1, 0.0f, 0.0f); }
    for (int i = 0; i < sc.plane_count(); i++) { if (!sc.plane_visible(i)) continue; P3 n; float dist; sc.plane(i, n, dist); offer(a, plane_d2(p, n, dist), KIND_PLANE, i, -1, 0.0f, 0.0f); }
    if (sc.tlas_nodes() <= 0) return;
    int sp = 0, floor_sp = 0, cur = -1, first = 0, count = 0, tl_i = 0, tl_end = 0, inst = 0;
    bool in_blas = false;
    { P3 mn, mx; sc.tlas_node(0, mn, mx, first, count); if (box_d2(p, mn, mx) < a.d2) cur = 0; }
    for (;;) {
        if (cur < 0) {
            if (in_blas && sp == floor_sp) in_blas = false;               // this instance is done
            if (!in_blas && tl_i < tl_end) {                              // the next instance of the TLAS leaf
                if (!sc.instance_visible(tl_i)) { tl_i++; continue; }     // FILTER: hidden from this row
                inst = sc.enter(tl_i++, p, pl);
                P3 mn, mx; sc.blas_node(0, mn, mx, first, count);
                in_blas = true; floor_sp = sp;
                if (box_d2(pl, mn, mx) < a.d2) cur = 0;
                continue;
            }
            if (sp == 0) break;
            float d2n; int node;
            sp--; st.pop(sp, node, d2n);
            if (!(d2n < a.d2)) continue;
            cur = node;
            P3 mn, mx;
            if (in_blas) sc.blas_node(cur, mn, mx, first, count); else sc.tlas_node(cur, mn, mx, first, count);
        }
        if ((count & 0x3fffffff) > 0) {                                   // a leaf: (first, count) of node cur
            const int n = count & 0x3fffffff;
            if (in_blas) {
                for (int i = first; i < first + n; i++) {
                    P3 p0, e1, e2; float u, v;
                    sc.triangle(i, p0, e1, e2);
                    const float d2 = triangle_d2(sub(pl, p0), e1, e2, u, v);
                    offer(a, d2, KIND_TRI, inst, i, u, v);
                }
            } else { tl_i = first; tl_end = first + n; }
            cur = -1;
            continue;
        }
        P3 lmn, lmx, rmn, rmx; int lf, lc, rf, rc;
        const int left = first;
        if (in_blas) { sc.blas_node(left, lmn, lmx, lf, lc); sc.blas_node(left + 1, rmn, rmx, rf, rc); }
        else         { sc.tlas_node(left, lmn, lmx, lf, lc); sc.tlas_node(left + 1, rmn, rmx, rf, rc); }
        const P3 q = in_blas ? pl : p;
        const float dl = box_d2(q, lmn, lmx), dr = box_d2(q, rmn, rmx);
        const bool left_first = dl <= dr;
        const float d_near = left_first ? dl : dr, d_far = left_first ? dr : dl;
        if (d_far < a.d2) { st.push(sp, left_first ? left + 1 : left, d_far); sp++; }
        if (d_near < a.d2) { cur = left_first ? left : left + 1; first = left_first ? lf : rf; count = left_first ? lc : rc; }
        else cur = -1;
    }
}

}  // namespace rtxnp
