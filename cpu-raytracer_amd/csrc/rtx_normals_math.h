// rtx_normals_math.h — the arithmetic of the device-side vertex normals (rtx_blas_vertex_normals), written once and compiled twice like
// rtx_refit_math.h: by hipcc into the kernels of rtx_normals.h and by the host compiler into rtxh_vertex_normals (host/rtx_host.cpp) and
// normals_check.cpp.  Unfused fp32, correctly rounded '/' and sqrtf on both sides, so the bits agree.  Plain C++: no HIP types.
//
// Smooth, area-weighted vertex normals (Device-side vertex normals):
//   valid     a triangle is valid when its three indices lie in [0, vertex_count) — rtx_build_blas's rule, -1 pads a mesh.  Nothing is read
//             through the indices of an invalid triangle and it contributes to no vertex.
//   face      e1 = p1 - p0, e2 = p2 - p0, f = e1 x e2 (length = twice the area).  A face vector with a NaN or infinite component is
//             replaced by (+0, +0, +0): a bad vertex spoils its own normal and never a neighbour's.
//   sum       from (+0, +0, +0), the face vector added once for every corner c = 3 * t + k that holds the vertex, in ascending c.  The order
//             is part of the specification: it is the order of a plain loop over triangles and corners.
//   normal    m = max(|x|, |y|, |z|) of the sum; m zero or not finite (a sum with a NaN or infinite component): (+0, +0, +0); otherwise
//             a = s / m, d = a.x * a.x + (a.y * a.y + a.z * a.z), n = a / sqrtf(d) — at any scale, since |a| <= 1 with one component +-1.
//             A vertex no valid triangle uses, and a vertex whose contributions cancel, get (+0, +0, +0).
//   index     the key of corner c is (uint64)v << 32 | c, v the vertex at that corner, v = vertex_count for a corner of an invalid
//             triangle (it sorts last).  A total order: any correct sort gives one result.  offset[v], v in [0, vertex_count], is the lower
//             bound of v << 32 in the sorted keys; the corners of vertex v are sorted[offset[v] .. offset[v + 1]).
#pragma once
#include "rtx_update_math.h"

#define RTX_NORMALS_MAX_TRIANGLES (1 << 28)      // include/rtx.h; the corner index 3 * t + k and rocPRIM's count are 32-bit

namespace rtxn {

RTX_HD bool valid_triangle(int32_t i0, int32_t i1, int32_t i2, int32_t vertex_count) {
    return i0 >= 0 && i0 < vertex_count && i1 >= 0 && i1 < vertex_count && i2 >= 0 && i2 < vertex_count;
}

// the sort key of corner c of a triangle with the indices tri[0 .. 3)
RTX_HD uint64_t corner_key(const int32_t tri[3], uint32_t c, int32_t vertex_count) {
    const uint32_t v = valid_triangle(tri[0], tri[1], tri[2], vertex_count) ? (uint32_t)tri[c % 3u] : (uint32_t)vertex_count;
    return (uint64_t)v << 32 | c;
}

// the key bits a sort has to look at: 32 of the corner and those of v in [0, vertex_count]
RTX_HD unsigned int key_bits(int32_t vertex_count) {
    unsigned int b = 0;
    while (b < 32 && ((uint32_t)vertex_count >> b) != 0) b++;
    return 32 + b;
}

// the first position in keys[0, n) whose key is >= key: one probe per halving, so every lane of a launch takes the same number of steps
// (bit length of n: at most 30 for n = 3 * 2^28) whatever the data
RTX_HD uint32_t lower_bound(const uint64_t * keys, uint32_t n, uint64_t key) {
    uint32_t lo = 0, len = n;
    while (len > 0) {
        const uint32_t half = len >> 1;
        if (keys[lo + half] < key) { lo += half + 1; len -= half + 1; } else len = half;
    }
    return lo;
}

RTX_HD void face_vector(const float p0[3], const float p1[3], const float p2[3], float f[3]) {
    float e1[3], e2[3];
    for (int a = 0; a < 3; a++) { e1[a] = p1[a] - p0[a]; e2[a] = p2[a] - p0[a]; }
    f[0] = e1[1] * e2[2] - e1[2] * e2[1];
    f[1] = e1[2] * e2[0] - e1[0] * e2[2];
    f[2] = e1[0] * e2[1] - e1[1] * e2[0];
    if (!(rtxu::is_finite(f[0]) && rtxu::is_finite(f[1]) && rtxu::is_finite(f[2]))) { f[0] = 0.0f; f[1] = 0.0f; f[2] = 0.0f; }
}

// pass 1: the face vector of triangle t of the index table, zeros for an invalid one
RTX_HD void triangle_face(const int32_t * indices, const float * positions, uint32_t t, int32_t vertex_count, float f[3]) {
    const int32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
    f[0] = 0.0f; f[1] = 0.0f; f[2] = 0.0f;
    if (!valid_triangle(i0, i1, i2, vertex_count)) return;
    const float * const q0 = positions + 3 * (size_t)i0, * const q1 = positions + 3 * (size_t)i1, * const q2 = positions + 3 * (size_t)i2;
    const float p0[3] = { q0[0], q0[1], q0[2] }, p1[3] = { q1[0], q1[1], q1[2] }, p2[3] = { q2[0], q2[1], q2[2] };
    face_vector(p0, p1, p2, f);
}

RTX_HD void normalise(const float s[3], float n[3]) {
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    if (!(rtxu::is_finite(s[0]) && rtxu::is_finite(s[1]) && rtxu::is_finite(s[2]))) return;
    const float ax = fabsf(s[0]), ay = fabsf(s[1]), az = fabsf(s[2]);
    float m = ax > ay ? ax : ay;
    m = m > az ? m : az;
    if (m == 0.0f) return;
    const float a[3] = { s[0] / m, s[1] / m, s[2] / m };
    const float d = a[0] * a[0] + (a[1] * a[1] + a[2] * a[2]);
    const float l = sqrtf(d);
    n[0] = a[0] / l; n[1] = a[1] / l; n[2] = a[2] / l;
}

// pass 2: the normal of the vertex whose corners are sorted[begin, end), from the stored face vectors (Face: .x .y .z, one per triangle).
// Four corners at a time: the eight loads of a batch do not depend on one another, so a long list (the pole of a UV sphere) is not one
// chain of 2 * valence dependent loads; the additions stay one by one in ascending corner order, which is what fixes the bits.
template <typename Face> RTX_HD void vertex_normal(const uint64_t * sorted, uint32_t begin, uint32_t end, const Face * face, float n[3]) {
    float s[3] = { 0.0f, 0.0f, 0.0f };
    uint32_t k = begin;
    for (; end - k >= 4u; k += 4u) {
        const uint32_t c0 = (uint32_t)sorted[k], c1 = (uint32_t)sorted[k + 1], c2 = (uint32_t)sorted[k + 2], c3 = (uint32_t)sorted[k + 3];
        const Face f0 = face[c0 / 3u], f1 = face[c1 / 3u], f2 = face[c2 / 3u], f3 = face[c3 / 3u];
        s[0] += f0.x; s[1] += f0.y; s[2] += f0.z;
        s[0] += f1.x; s[1] += f1.y; s[2] += f1.z;
        s[0] += f2.x; s[1] += f2.y; s[2] += f2.z;
        s[0] += f3.x; s[1] += f3.y; s[2] += f3.z;
    }
    for (; k < end; k++) {
        const Face f = face[(uint32_t)sorted[k] / 3u];
        s[0] += f.x; s[1] += f.y; s[2] += f.z;
    }
    normalise(s, n);
}

}  // namespace rtxn
