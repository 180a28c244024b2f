// rtx_update_math.h — the arithmetic of the device-side scene update (rtx_update_instances), written once and compiled twice: by hipcc
// into the kernels of rtx_update.h and by the host compiler into rtxh_tlas_build_balanced (host/rtx_host.cpp), which is the specification
// the device tree is compared with.  Both builds use unfused fp32 (-ffp-contract=off) and a correctly rounded division, so every function
// here returns the same bits on the CPU and on gfx950.  Plain C++: no HIP types, no libm beyond fabsf.
//
// The balanced TLAS ("a tree of this project's own", DESIGN.md 3, Device-side scene update):
//   * instances sorted by (world AABB finite?, 30-bit Morton code of their position, instance index): a total order, so any correct sort
//     gives one result; instances with a non-finite box come first (see sort_key);
//   * an implicit heap over the sorted range: node (d, j), j < 2^d, covers sorted slots [j*n >> d, (j+1)*n >> d) and is a leaf when that
//     is one slot; it is stored at index 2^d + j, the root at 0 — children adjacent at `left`, `left + 1`, index 1 unused, as in the
//     reference's arrays (BVHBuilders.h:8-46).  Shape, node count (2 << L) and depth depend on n alone; slots under a leaf above the last
//     level are holes (all zero bytes), which no traversal can reach.
//   * boxes bottom-up from the STORED child boxes, so a parent encloses its children in the stored floats.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define RTX_HD __host__ __device__ inline
#else
#define RTX_HD inline
#endif

#ifndef RTX_UPDATE_MAX_INSTANCES
#define RTX_UPDATE_MAX_INSTANCES 65536      // include/rtx.h; the instance index takes the low 16 bits of a sort key
#endif

namespace rtxu {

struct Box { float mn[3], mx[3]; };

// ---- Mesh::update (Mesh.cpp:9-15), expression for expression what host/rtx_host.cpp evaluates ----------------------------------------
// Transform::calc_world_matrix, Transform.h:13-43; cells[i + 4*j] (Matrix4.h:19-23)
RTX_HD void world_matrix(const float p[3], const float r[4], float * c) {
    for (int i = 0; i < 16; i++) c[i] = 0.0f;
    c[15] = 1.0f;
    const float xx = r[0] * r[0], yy = r[1] * r[1], zz = r[2] * r[2];
    const float xz = r[0] * r[2], xy = r[0] * r[1], yz = r[1] * r[2];
    const float wx = r[3] * r[0], wy = r[3] * r[1], wz = r[3] * r[2];
    c[0] = 1.0f - 2.0f * (yy + zz); c[4] = 2.0f * (xy + wz);        c[8]  = 2.0f * (xz - wy);
    c[1] = 2.0f * (xy - wz);        c[5] = 1.0f - 2.0f * (xx + zz); c[9]  = 2.0f * (yz + wx);
    c[2] = 2.0f * (xz + wy);        c[6] = 2.0f * (yz - wx);        c[10] = 1.0f - 2.0f * (xx + yy);
    c[3] = p[0]; c[7] = p[1]; c[11] = p[2];
}

// one cofactor of Matrix4::invert (Matrix4.h:88-138): six signed triple products summed left to right; s = the signs (bit t set: minus)
#define RTXU_T(sg, a, b, c_) ((sg) ? -m[a] : m[a]) * m[b] * m[c_]
RTX_HD void invert(const float * m, float * out) {
    float inv[16];
    inv[0]  = RTXU_T(0, 5, 10, 15) + RTXU_T(1, 5, 11, 14) + RTXU_T(1, 9, 6, 15) + RTXU_T(0, 9, 7, 14) + RTXU_T(0, 13, 6, 11) + RTXU_T(1, 13, 7, 10);
    inv[1]  = RTXU_T(1, 1, 10, 15) + RTXU_T(0, 1, 11, 14) + RTXU_T(0, 9, 2, 15) + RTXU_T(1, 9, 3, 14) + RTXU_T(1, 13, 2, 11) + RTXU_T(0, 13, 3, 10);
    inv[2]  = RTXU_T(0, 1, 6, 15) + RTXU_T(1, 1, 7, 14) + RTXU_T(1, 5, 2, 15) + RTXU_T(0, 5, 3, 14) + RTXU_T(0, 13, 2, 7) + RTXU_T(1, 13, 3, 6);
    inv[3]  = RTXU_T(1, 1, 6, 11) + RTXU_T(0, 1, 7, 10) + RTXU_T(0, 5, 2, 11) + RTXU_T(1, 5, 3, 10) + RTXU_T(1, 9, 2, 7) + RTXU_T(0, 9, 3, 6);
    inv[4]  = RTXU_T(1, 4, 10, 15) + RTXU_T(0, 4, 11, 14) + RTXU_T(0, 8, 6, 15) + RTXU_T(1, 8, 7, 14) + RTXU_T(1, 12, 6, 11) + RTXU_T(0, 12, 7, 10);
    inv[5]  = RTXU_T(0, 0, 10, 15) + RTXU_T(1, 0, 11, 14) + RTXU_T(1, 8, 2, 15) + RTXU_T(0, 8, 3, 14) + RTXU_T(0, 12, 2, 11) + RTXU_T(1, 12, 3, 10);
    inv[6]  = RTXU_T(1, 0, 6, 15) + RTXU_T(0, 0, 7, 14) + RTXU_T(0, 4, 2, 15) + RTXU_T(1, 4, 3, 14) + RTXU_T(1, 12, 2, 7) + RTXU_T(0, 12, 3, 6);
    inv[7]  = RTXU_T(0, 0, 6, 11) + RTXU_T(1, 0, 7, 10) + RTXU_T(1, 4, 2, 11) + RTXU_T(0, 4, 3, 10) + RTXU_T(0, 8, 2, 7) + RTXU_T(1, 8, 3, 6);
    inv[8]  = RTXU_T(0, 4, 9, 15) + RTXU_T(1, 4, 11, 13) + RTXU_T(1, 8, 5, 15) + RTXU_T(0, 8, 7, 13) + RTXU_T(0, 12, 5, 11) + RTXU_T(1, 12, 7, 9);
    inv[9]  = RTXU_T(1, 0, 9, 15) + RTXU_T(0, 0, 11, 13) + RTXU_T(0, 8, 1, 15) + RTXU_T(1, 8, 3, 13) + RTXU_T(1, 12, 1, 11) + RTXU_T(0, 12, 3, 9);
    inv[10] = RTXU_T(0, 0, 5, 15) + RTXU_T(1, 0, 7, 13) + RTXU_T(1, 4, 1, 15) + RTXU_T(0, 4, 3, 13) + RTXU_T(0, 12, 1, 7) + RTXU_T(1, 12, 3, 5);
    inv[11] = RTXU_T(1, 0, 5, 11) + RTXU_T(0, 0, 7, 9) + RTXU_T(0, 4, 1, 11) + RTXU_T(1, 4, 3, 9) + RTXU_T(1, 8, 1, 7) + RTXU_T(0, 8, 3, 5);
    inv[12] = RTXU_T(1, 4, 9, 14) + RTXU_T(0, 4, 10, 13) + RTXU_T(0, 8, 5, 14) + RTXU_T(1, 8, 6, 13) + RTXU_T(1, 12, 5, 10) + RTXU_T(0, 12, 6, 9);
    inv[13] = RTXU_T(0, 0, 9, 14) + RTXU_T(1, 0, 10, 13) + RTXU_T(1, 8, 1, 14) + RTXU_T(0, 8, 2, 13) + RTXU_T(0, 12, 1, 10) + RTXU_T(1, 12, 2, 9);
    inv[14] = RTXU_T(1, 0, 5, 14) + RTXU_T(0, 0, 6, 13) + RTXU_T(0, 4, 1, 14) + RTXU_T(1, 4, 2, 13) + RTXU_T(1, 12, 1, 6) + RTXU_T(0, 12, 2, 5);
    inv[15] = RTXU_T(0, 0, 5, 10) + RTXU_T(1, 0, 6, 9) + RTXU_T(1, 4, 1, 10) + RTXU_T(0, 4, 2, 9) + RTXU_T(0, 8, 1, 6) + RTXU_T(1, 8, 2, 5);
    for (int i = 0; i < 16; i++) out[i] = 0.0f;
    out[0] = out[5] = out[10] = out[15] = 1.0f;
    const float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det != 0.0f) {
        const float inv_det = 1.0f / det;
        for (int i = 0; i < 16; i++) out[i] = inv[i] * inv_det;
    }
}
#undef RTXU_T

// ---- rigid poses: what the length queries accept (include/rtx.h, rtx_query_nearest: Limits) --------------------------------------------------
// A matrix is rigid when its linear part R (rows c[4a .. 4a+2]) is orthogonal within RTXU_RIGID_TAU: every |(R.R^T - I)ij| <= tau, in fp64
// from the fp32 cells (a NaN or infinite cell fails every comparison: not rigid).  A reflection is orthogonal and passes.  An instance is
// rigid when both its world and its world_inv are.  tau = 2^-12 is a measurement (Non-rigid matrices): the power of two at
// least four times the largest deviation over 10^5 random fp32 unit quaternions through world_matrix / invert above (7.2e-7) and over every
// scene the suite builds (3.9e-5: poses scripted with a five-decimal axis, which Quaternion::axis_angle does not normalise).  Host code
// only: rtx_set_frame and rtxh_instances_rigid compile this one definition.
#define RTXU_RIGID_TAU (1.0 / 4096.0)
inline double rigid_deviation(const float * c) {
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) {
            double s = i == j ? -1.0 : 0.0;
            for (int k = 0; k < 3; k++) s += (double)c[4 * i + k] * (double)c[4 * j + k];
            const double a = s < 0.0 ? -s : s;
            if (a != a) return a;                           // a NaN cell: the deviation is a NaN, which no comparison accepts
            if (a > worst) worst = a;
        }
    return worst;
}
inline bool matrix_rigid(const float * c) { return rigid_deviation(c) <= RTXU_RIGID_TAU; }
inline bool instance_rigid(const float * world, const float * world_inv) { return matrix_rigid(world) && matrix_rigid(world_inv); }
inline bool matrix_finite(const float * c) {
    bool f = true;
    for (int i = 0; i < 16; i++) { uint32_t u; __builtin_memcpy(&u, c + i, 4); f = f && (u & 0x7f800000u) != 0x7f800000u; }
    return f;
}

// AABB::transform (AABB.cpp:55-73) of the BLAS root box by the world matrix w
RTX_HD Box transform_box(const float * w, const float mn[3], const float mx[3]) {
    float ce[3], ex[3];
    for (int a = 0; a < 3; a++) { ce[a] = 0.5f * (mn[a] + mx[a]); ex[a] = 0.5f * (mx[a] - mn[a]); }
    Box b;
    for (int a = 0; a < 3; a++) {
        const float * r = w + 4 * a;
        const float nc = r[0] * ce[0] + r[1] * ce[1] + r[2] * ce[2] + r[3];                     // Matrix4::transform_position
        const float ne = fabsf(r[0]) * ex[0] + fabsf(r[1]) * ex[1] + fabsf(r[2]) * ex[2];       // Matrix4::abs + transform_direction
        b.mn[a] = nc - ne; b.mx[a] = nc + ne;
    }
    return b;
}

// AABB::fix_if_needed, AABB.h:26-32
RTX_HD void fix_if_needed(Box & b) {
    for (int a = 0; a < 3; a++) if (b.mx[a] - b.mn[a] < 0.001f) b.mx[a] += 0.005f;
}

// ---- sort keys ------------------------------------------------------------------------------------------------------------------------
// a float as an unsigned integer with the same order (-inf < ... < -0 < +0 < ... < +inf); the bounds of the positions are min / max
// reductions over these, which — unlike float min / max with NaN or signed zeros — give one result in any order
RTX_HD uint32_t ordered_key(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
RTX_HD float ordered_value(uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; __builtin_memcpy(&f, &u, 4); return f; }
RTX_HD bool is_finite(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return (u & 0x7f800000u) != 0x7f800000u; }
#define RTXU_KEY_LO_INIT 0xff800000u     // ordered_key(+inf): the bounds when no position component is finite
#define RTXU_KEY_HI_INIT 0x007fffffu     // ordered_key(-inf)
// the bounds as sort_key wants them, from six min-reduced keys (lo.xyz as they are, hi.xyz complemented; 0xffffffff before the reduction): a
// reduction nothing took part in (no finite coordinate on that axis) still holds its initial value
RTX_HD void reduced_bounds(const uint32_t * bounds, uint32_t b6[6]) {
    for (int a = 0; a < 3; a++) {
        const uint32_t lo = bounds[a], hc = bounds[3 + a];
        b6[a] = lo == 0xffffffffu ? RTXU_KEY_LO_INIT : lo; b6[3 + a] = hc == 0xffffffffu ? RTXU_KEY_HI_INIT : ~hc;
    }
}

// one coordinate -> one of 1024 cells between the bounds of the finite coordinates of that axis.  Clamped; a NaN (a NaN coordinate, or
// 0 / 0 when all coordinates are equal) is cell 0, so every float input has a cell and no conversion is out of range.
RTX_HD uint32_t cell_of(float p, float lo, float hi) {
    const float t = (p - lo) / (hi - lo);
    if (!(t >= 0.0f)) return 0u;
    if (t >= 1.0f) return 1023u;
    const uint32_t q = (uint32_t)(t * 1024.0f);
    return q > 1023u ? 1023u : q;
}
RTX_HD uint32_t spread10(uint32_t v) {       // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000ffu; v = (v | (v << 8)) & 0x0300f00fu; v = (v | (v << 4)) & 0x030c30c3u; v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// bounds6: ordered keys of (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z)
// Bit 46: the instance's world AABB is finite.  Instances with a NaN or infinite box component sort FIRST, whatever their position.  An
// inner box takes a NaN only from its right child (`l < r ? l : r` returns r when either is a NaN), so a NaN inner box ends in a
// non-finite rightmost leaf, and with those leaves in the lowest slots everything under it is non-finite too: a bad pose can hide its own
// instance, never a neighbour whose pose is fine.
RTX_HD bool box_is_finite(const Box & b) { bool f = true; for (int a = 0; a < 3; a++) f = f && is_finite(b.mn[a]) && is_finite(b.mx[a]); return f; }
RTX_HD uint64_t sort_key(const float p[3], const uint32_t bounds6[6], uint32_t index, bool finite_box) {
    uint32_t code = 0;
    for (int a = 0; a < 3; a++) code |= spread10(cell_of(p[a], ordered_value(bounds6[a]), ordered_value(bounds6[3 + a]))) << (2 - a);
    return ((uint64_t)(finite_box ? 1 : 0) << 46) | ((uint64_t)code << 16) | (uint64_t)index;
}
#define RTXU_KEY_BITS 47

// ---- shape of the tree: functions of n alone --------------------------------------------------------------------------------------------
RTX_HD int tree_levels(int n) { int L = 0; while ((1 << L) < n) L++; return L; }             // L = ceil(log2 n): the deepest level that holds a node
RTX_HD int tree_node_count(int n) { return 2 << tree_levels(n); }                            // slots, holes and index 1 included
RTX_HD int tree_inner_depth(int n) { return n < 2 ? -1 : tree_levels(n) - 1; }              // depth of the deepest inner node (validate_tree's figure)
RTX_HD int range_first(int n, int d, int j) { return (int)(((int64_t)j * n) >> d); }
// node (d, j): count = sorted slots it covers, or 0 when the slot is a hole (its parent is a leaf, or it is beyond the tree)
RTX_HD int node_range(int n, int d, int j, int * first) {
    const int a = range_first(n, d, j), cnt = range_first(n, d, j + 1) - a;
    *first = a;
    if (d == 0) return cnt;
    const int pa = range_first(n, d - 1, j >> 1), pcnt = range_first(n, d - 1, (j >> 1) + 1) - pa;
    return pcnt >= 2 ? cnt : 0;
}
RTX_HD int node_slot(int d, int j) { return d == 0 ? 0 : (1 << d) + j; }

// an inner node from its children's stored boxes, left child first: the reference's `a < b ? a : b` forms (Math.h / Vector3::min, max), then
// fix_if_needed.  *axis (1..3, bits 30-31 of `count`, BVHNode::should_visit_left_first): the topology is fixed, so the children cannot be
// swapped; the axis is the one on which the right child's box centre lies furthest beyond the left child's (sums instead of centres: the
// same order), so that "left first when the ray travels in +axis" holds wherever the Morton order leaves an axis on which it can hold.
RTX_HD Box join_boxes(const Box & l, const Box & r, int * axis) {
    Box b;
    for (int a = 0; a < 3; a++) { b.mn[a] = l.mn[a] < r.mn[a] ? l.mn[a] : r.mn[a]; b.mx[a] = l.mx[a] > r.mx[a] ? l.mx[a] : r.mx[a]; }
    fix_if_needed(b);
    float best = (r.mn[0] + r.mx[0]) - (l.mn[0] + l.mx[0]); int ax = 1;
    for (int a = 1; a < 3; a++) { const float d = (r.mn[a] + r.mx[a]) - (l.mn[a] + l.mx[a]); if (d > best) { best = d; ax = a + 1; } }
    *axis = ax;
    return b;
}

}  // namespace rtxu
