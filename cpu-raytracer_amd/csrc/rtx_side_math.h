// rtx_side_math.h — the arithmetic of signed-distance queries (include/rtx.h: rtx_blas_pseudonormals, rtx_query_signed_distance): the
// angle-weighted pseudonormals of a mesh (Baerentzen and Aanaes, "Signed distance computation using the angle weighted pseudonormal", 2005)
// and the sign rule of a nearest-point answer.  Written once and compiled twice like rtx_nearest_math.h: by hipcc into the kernels of
// rtx_side.h and into k_query_nearest<.., SIGNED> (rtx_nearest.h), and by the host compiler into rtxh_blas_pseudonormals /
// rtxh_query_signed_distance (host/rtx_host.cpp) and side_check.cpp.  Unfused fp32 (-ffp-contract=off), correctly rounded '/' and sqrtf on
// both sides, atan2 from rtx_libm.h, every sum of three products in the order x + (y + z).  So every function here returns the same bits on
// the CPU and on gfx950.  Plain C++: no HIP types.  This comment is the specification.
//
// REGION   triangle_region(ap, e1, e2): the feature of triangle (p0, e1, e2) that holds the point nearest to p0 + ap — 0, 1, 2: vertex a, b,
//          c; 3, 4, 5: edge ab, bc, ac; 6: the face.  It is the return value of rtxnp::triangle_weights, the one place the conditional chain
//          of TRIANGLE (rtx_nearest_math.h) is written: by construction the branch rtxnp::triangle_d2 took, with its (u, v).
// TOPOLOGY the SOURCE index buffer of rtx_set_blas_topology: T triangles over V vertices, corner c = 3 t + k.  A triangle is valid when its
//          three indices lie in [0, V) (rtx_normals_math.h); the corner list of vertex v holds the corners of VALID triangles that name v, in
//          ascending c (the inverted index of rtx_set_blas_topology; on the host the order of a plain loop over triangles and corners).
// FACE     of source triangle t.  An invalid triangle: unit normal (+0, +0, +0), angles 0.  Otherwise f = e1 x e2 with e1 = p1 - p0,
//          e2 = p2 - p0 as rtxn::face_vector spells it (a NaN or infinite component: f = (+0, +0, +0)), normalised by the max-component rule
//          of the vertex normals (rtxn::normalise): m = max(|x|, |y|, |z|), a = f / m, l = sqrtf(a.x*a.x + (a.y*a.y + a.z*a.z)), n = a / l —
//          a unit vector at any scale.  m == 0: n = (+0, +0, +0) and the three corner angles are 0.  The length L = m * l is computed once
//          per triangle.
// ANGLE    at corner k of a triangle with L > 0: rtx_atan2f(L, ea . eb), ea and eb the two edges that leave the corner (corner 0: p1 - p0,
//          p2 - p0; corner 1: p2 - p1, p0 - p1; corner 2: p0 - p2, p1 - p2).  In [0, pi]; a non-finite angle (a dot product that overflowed
//          to NaN) is 0.  The corner vector is angle * n per component.
// VERTEX   vert_pn[v] = the sum, from (+0, +0, +0), of the corner vectors of v's corner list in ascending c, added one by one.  Not
//          normalised: only its direction's sign is ever used.  A sum with a non-finite component becomes (+0, +0, +0).  A vertex no valid
//          triangle uses gets (+0, +0, +0).
// EDGE     edge_pn[3 s + k] of slot s (a triangle slot of the BLAS, vertices (a, b, c) = slot_vertices[3 s ..]): k = 0, 1, 2 is edge ab, bc,
//          ac, between the vertices (x, y) = (a, b), (b, c), (a, c).  It is the sum, from (+0, +0, +0), over the corners c of x's list in
//          ascending c, of the unit normal of source triangle c / 3, for every such triangle that also has y at one of its corners.  So a
//          boundary edge gets its one face's unit normal bit for bit, a manifold edge the sum of two, a non-manifold edge the sum of all,
//          two coincident opposite faces zero; a slot of an SBVH that repeats a source triangle gets the record of its twin, because the
//          lists are over the source topology and not over the slots.  x or y outside [0, V) (-1: a pad slot of rtx_build_blas): zeros.  A
//          non-finite sum becomes zeros.  No table component is ever NaN or infinite.
// SIDE     of the walk's winner (instance, slot) at the local point p_l = xform_pos(world_inv, p) — the walk's own: ap = p_l - p0, then the
//          region and (u, v) of triangle_weights, w = e1*u + e2*v, r = ap - w: exactly the values triangle_d2 had.  N is
//            face     e1 x e2 of the hot record (the slot's own orientation; no table is read),
//            edge k   edge_pn[3 slot + k],
//            vertex k vert_pn[slot_vertices[3 slot + k]] (an index outside [0, V): zeros).
//          The distance is NEGATIVE iff r . N < 0 (x + (y + z)).  Everything else is positive: r . N == 0, a zero N, a NaN.  The signed
//          distance is sqrtf(d2) with that sign, and +0 when d2 == 0.  r and N are both local, so a rigid, scaled or mirrored instance needs
//          no world transform: a mirrored instance mirrors r and the mesh alike.
//          SPHERE  negative iff l < r, with l = sqrtf(v.v) and r = sqrtf(radius_squared), the two roots sphere_d2 takes.
//          PLANE   negative iff n.p + distance < 0.
//          A dead, invisible or unanswered row: +INFINITY, feature 0.
// FEATURE  one int32 per row: 0 none, 1 face, 2 edge, 3 vertex, 4 sphere, 5 plane; + 8 (FEATURE_NAIVE) when the winning mesh has no tables:
//          then N = e1 x e2 in every region, and the flag tells the caller that the sign near edges and vertices is the naive one.
// LIMITS   The sign is relative to the OBJECT that owns the nearest point: for overlapping solids it is not the sign of their union.  For a
//          closed, consistently oriented mesh negative means inside; for an open one it is the side of the surface.  The tables are as
//          current as the last rtx_blas_pseudonormals call: a refit or a rebuild without that call leaves them stale — the contract the
//          vertex normals have.  Within the distance bound of rtx_nearest_math.h of a surface, and where r is within rounding of
//          perpendicular to N, the sign is not determined.
#pragma once
#include "rtx_nearest_math.h"
#include "rtx_normals_math.h"

namespace rtxsd {

using rtxnp::P3;
enum { FEATURE_NONE = 0, FEATURE_FACE = 1, FEATURE_EDGE = 2, FEATURE_VERTEX = 3, FEATURE_SPHERE = 4, FEATURE_PLANE = 5, FEATURE_NAIVE = 8 };
#define RTX_SIDE_RECORD 4          // float4 per source triangle: the unit normal, then the three corner vectors (w: the corner's angle)

// REGION
RTX_HDF int triangle_region(P3 ap, P3 e1, P3 e2) { float u, v; return rtxnp::triangle_weights(ap, e1, e2, u, v); }
RTX_HDF int region_feature(int region) { return region == rtxnp::REGION_FACE ? FEATURE_FACE : region >= rtxnp::REGION_EDGE_AB ? FEATURE_EDGE : FEATURE_VERTEX; }

// FACE: the unit normal of face vector f (rtxn::normalise's expressions) and its length; zeros and 0 for a zero vector
RTX_HD float face_unit(const float f[3], float n[3]) {
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    if (!(rtxu::is_finite(f[0]) && rtxu::is_finite(f[1]) && rtxu::is_finite(f[2]))) return 0.0f;
    const float ax = fabsf(f[0]), ay = fabsf(f[1]), az = fabsf(f[2]);
    float m = ax > ay ? ax : ay;
    m = m > az ? m : az;
    if (m == 0.0f) return 0.0f;
    const float a[3] = { f[0] / m, f[1] / m, f[2] / m };
    const float d = a[0] * a[0] + (a[1] * a[1] + a[2] * a[2]);
    const float l = sqrtf(d);
    n[0] = a[0] / l; n[1] = a[1] / l; n[2] = a[2] / l;
    return m * l;
}
// ANGLE at the corner whose leaving edges are (q1 - q0) and (q2 - q0), L = the face vector's length (> 0)
RTX_HD float corner_angle(const float q0[3], const float q1[3], const float q2[3], float L) {
    const float ea[3] = { q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2] }, eb[3] = { q2[0] - q0[0], q2[1] - q0[1], q2[2] - q0[2] };
    const float c = ea[0] * eb[0] + (ea[1] * eb[1] + ea[2] * eb[2]);
    const float a = rtx_atan2f(L, c);
    return rtxu::is_finite(a) ? a : 0.0f;
}
// the record of source triangle t: rec[0 .. 3) the unit normal, rec[4 + 4 k .. 4 + 4 k + 3) corner vector k and its angle; 16 floats
RTX_HD void triangle_record(const int32_t * indices, const float * positions, uint32_t t, int32_t vertex_count, float rec[16]) {
    for (int i = 0; i < 16; i++) rec[i] = 0.0f;
    const int32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
    if (!rtxn::valid_triangle(i0, i1, i2, vertex_count)) return;
    const float * const q0 = positions + 3 * (size_t)i0, * const q1 = positions + 3 * (size_t)i1, * const q2 = positions + 3 * (size_t)i2;
    const float p0[3] = { q0[0], q0[1], q0[2] }, p1[3] = { q1[0], q1[1], q1[2] }, p2[3] = { q2[0], q2[1], q2[2] };
    float f[3], n[3];
    rtxn::face_vector(p0, p1, p2, f);
    const float L = face_unit(f, n);
    rec[0] = n[0]; rec[1] = n[1]; rec[2] = n[2];
    if (!(L > 0.0f)) return;
    const float ang[3] = { corner_angle(p0, p1, p2, L), corner_angle(p1, p2, p0, L), corner_angle(p2, p0, p1, L) };
    for (int k = 0; k < 3; k++) { rec[4 + 4 * k] = ang[k] * n[0]; rec[5 + 4 * k] = ang[k] * n[1]; rec[6 + 4 * k] = ang[k] * n[2]; rec[7 + 4 * k] = ang[k]; }
}
// a finished sum: zeros when a component is not finite
RTX_HD void finish_sum(const float s[3], float out[4]) {
    const bool ok = rtxu::is_finite(s[0]) && rtxu::is_finite(s[1]) && rtxu::is_finite(s[2]);
    out[0] = ok ? s[0] : 0.0f; out[1] = ok ? s[1] : 0.0f; out[2] = ok ? s[2] : 0.0f; out[3] = 0.0f;
}

// VERTEX: the pseudonormal of the vertex whose corners are sorted[begin, end), from the stored records (Rec: .x .y .z .w, RTX_SIDE_RECORD per
// triangle).  Four corners at a time like rtxn::vertex_normal: the loads of a batch do not depend on one another, the additions stay one by
// one in ascending corner order.
template <typename Rec> RTX_HD void vertex_pseudonormal(const uint64_t * sorted, uint32_t begin, uint32_t end, const Rec * rec, float out[4]) {
    float s[3] = { 0.0f, 0.0f, 0.0f };
    uint32_t k = begin;
    for (; end - k >= 4u; k += 4u) {
        const uint32_t c0 = (uint32_t)sorted[k], c1 = (uint32_t)sorted[k + 1], c2 = (uint32_t)sorted[k + 2], c3 = (uint32_t)sorted[k + 3];
        const Rec f0 = rec[RTX_SIDE_RECORD * (size_t)(c0 / 3u) + 1u + c0 % 3u], f1 = rec[RTX_SIDE_RECORD * (size_t)(c1 / 3u) + 1u + c1 % 3u];
        const Rec f2 = rec[RTX_SIDE_RECORD * (size_t)(c2 / 3u) + 1u + c2 % 3u], f3 = rec[RTX_SIDE_RECORD * (size_t)(c3 / 3u) + 1u + c3 % 3u];
        s[0] += f0.x; s[1] += f0.y; s[2] += f0.z;
        s[0] += f1.x; s[1] += f1.y; s[2] += f1.z;
        s[0] += f2.x; s[1] += f2.y; s[2] += f2.z;
        s[0] += f3.x; s[1] += f3.y; s[2] += f3.z;
    }
    for (; k < end; k++) {
        const uint32_t c = (uint32_t)sorted[k];
        const Rec f = rec[RTX_SIDE_RECORD * (size_t)(c / 3u) + 1u + c % 3u];
        s[0] += f.x; s[1] += f.y; s[2] += f.z;
    }
    finish_sum(s, out);
}

// the two vertices of edge k of a slot with the vertices sv[0 .. 3)
RTX_HD void edge_vertices(const int32_t sv[3], int k, int32_t & x, int32_t & y) { x = sv[k == 1 ? 1 : 0]; y = sv[k == 0 ? 1 : 2]; }
RTX_HD bool has_vertex(const int32_t * tri, int32_t y) { return tri[0] == y || tri[1] == y || tri[2] == y; }

// EDGE: the pseudonormal of the edge (x, y) from x's corner list sorted[offset[x], offset[x + 1]) — indices: the topology's T x 3 table.  Two
// corners at a time: the index and record loads of a pair are independent, the additions in ascending corner order.
template <typename Rec> RTX_HD void edge_pseudonormal(const uint64_t * sorted, const uint32_t * offset, const int32_t * indices, const Rec * rec,
                                                      int32_t vertex_count, int32_t x, int32_t y, float out[4]) {
    float s[3] = { 0.0f, 0.0f, 0.0f };
    if (x >= 0 && x < vertex_count && y >= 0 && y < vertex_count) {
        uint32_t k = offset[x];
        const uint32_t end = offset[x + 1];
        for (; end - k >= 2u; k += 2u) {
            const uint32_t t0 = (uint32_t)sorted[k] / 3u, t1 = (uint32_t)sorted[k + 1] / 3u;
            const int32_t * const i0 = indices + 3 * (size_t)t0, * const i1 = indices + 3 * (size_t)t1;
            const int32_t a0[3] = { i0[0], i0[1], i0[2] }, a1[3] = { i1[0], i1[1], i1[2] };
            const Rec f0 = rec[RTX_SIDE_RECORD * (size_t)t0], f1 = rec[RTX_SIDE_RECORD * (size_t)t1];
            if (has_vertex(a0, y)) { s[0] += f0.x; s[1] += f0.y; s[2] += f0.z; }
            if (has_vertex(a1, y)) { s[0] += f1.x; s[1] += f1.y; s[2] += f1.z; }
        }
        for (; k < end; k++) {
            const uint32_t t = (uint32_t)sorted[k] / 3u;
            const int32_t * const i0 = indices + 3 * (size_t)t;
            const int32_t a0[3] = { i0[0], i0[1], i0[2] };
            const Rec f = rec[RTX_SIDE_RECORD * (size_t)t];
            if (has_vertex(a0, y)) { s[0] += f.x; s[1] += f.y; s[2] += f.z; }
        }
    }
    finish_sum(s, out);
}

// SIDE of a triangle answer.  Tables gives has_tables(), edge(i) -> P3 (record i of edge_pn), vertex(slot, k) -> P3 (vert_pn of vertex k of
// the slot; zeros for an index outside the table).  Returns the FEATURE code; negative = the distance's sign.
template <typename Tables> RTX_HDF int triangle_side(P3 ap, P3 e1, P3 e2, int slot, const Tables & tb, bool & negative) {
    float u, v;
    const int region = rtxnp::triangle_weights(ap, e1, e2, u, v);
    const P3 w = rtxnp::add(rtxnp::scale(e1, u), rtxnp::scale(e2, v));
    const P3 r = rtxnp::sub(ap, w);
    const bool tables = tb.has_tables();
    P3 N;
    if (region == rtxnp::REGION_FACE || !tables) N = rtxnp::mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    else if (region >= rtxnp::REGION_EDGE_AB) N = tb.edge(3 * slot + (region - rtxnp::REGION_EDGE_AB));
    else N = tb.vertex(slot, region);
    negative = rtxnp::dot(r, N) < 0.0f;
    return region_feature(region) + (tables ? 0 : (int)FEATURE_NAIVE);
}
RTX_HDF bool sphere_side(P3 p, P3 c, float radius_squared) { const P3 v = rtxnp::sub(p, c); return rtxnp::root(rtxnp::dot(v, v)) < rtxnp::root(radius_squared); }
RTX_HDF bool plane_side(P3 p, P3 n, float distance) { return rtxnp::dot(n, p) + distance < 0.0f; }
// the signed distance of an answer with the squared distance d2
RTX_HDF float signed_distance(float d2, bool negative) { const float d = rtxnp::root(d2); return d2 == 0.0f ? 0.0f : negative ? -d : d; }

}  // namespace rtxsd
