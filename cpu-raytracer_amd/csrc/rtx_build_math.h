// rtx_build_math.h — the arithmetic of the device-side mesh build (rtx_alloc_blas / rtx_build_blas), written once and compiled twice like
// rtx_update_math.h and rtx_refit_math.h: by hipcc into the kernels of rtx_build.h and by the host compiler into rtxh_blas_build_balanced
// (host/rtx_host.cpp), the specification the device arrays are compared with.  Unfused fp32 on both sides.
//
// The balanced BLAS (Device-side mesh build):
//   * triangles sorted by (valid and box finite?, 30-bit Morton code of the centre of their box, source triangle index): a total order, so
//     any correct sort gives one permutation.  A triangle is VALID when its three indices lie in [0, vertex_count); its box is
//     rtxr::triangle_box, which is finite unless an axis has no finite component.  Triangles without the bit take Morton code 0 and sort first
//     in index order; they take no part in the bounds of the centres;
//   * an implicit heap over the sorted range, as in the balanced TLAS: node (d, j) covers sorted slots [j*n >> d, (j+1)*n >> d), is a leaf
//     when that is at most RTX_BUILD_LEAF_MAX slots and is stored at index 2^d + j (root at 0, index 1 unused, children adjacent, `left`
//     even).  Shape, node count and depth depend on n alone; slots that are no node are zero bytes;
//   * boxes by the refit's rules (rtx_refit_math.h), bottom-up from the STORED child boxes; an invalid triangle is skipped in its leaf;
//   * bits 30-31 of an inner node's `count`: the axis on which the right child's box centre lies furthest beyond the left child's (the
//     balanced TLAS's rule: the topology is fixed, children cannot be swapped).
#pragma once
#include "rtx_refit_math.h"

#define RTX_BUILD_LEAF_MAX      4            // triangles per leaf at most; must stay below the 16 of build_nodes_pk4c (rtx_layout_host.h)
#define RTX_BUILD_MAX_TRIANGLES (1 << 24)    // exclusive: the wide walks pack triangle and node indices into 24 bits
#define RTXB_INDEX_BITS 24                   // the source triangle index in the low bits of a sort key
#define RTXB_KEY_BITS   55                   // index + 30 bits of Morton code + the valid bit

namespace rtxb {

using rtxu::Box;

// ---- shape of the tree: functions of n alone ---------------------------------------------------------------------------------------------
// L = the deepest level that holds a node: the first level on which the largest range, ceil(n / 2^L) slots, fits a leaf
RTX_HD int tree_levels(int n) { int L = 0; while ((int)(((int64_t)n + ((int64_t)1 << L) - 1) >> L) > RTX_BUILD_LEAF_MAX) L++; return L; }
RTX_HD int tree_node_count(int n) { return 2 << tree_levels(n); }                            // slots, holes and index 1 included
RTX_HD int tree_inner_depth(int n) { return tree_levels(n) - 1; }                            // depth of the deepest inner node; -1: the root is a leaf
// node (d, j): count = sorted slots it covers, or 0 when the slot is a hole (its parent is a leaf; ranges only shrink downwards, so every
// ancestor of a node whose parent is inner is inner too)
RTX_HD int node_range(int n, int d, int j, int * first) {
    const int a = rtxu::range_first(n, d, j), cnt = rtxu::range_first(n, d, j + 1) - a;
    *first = a;
    if (d == 0) return cnt;
    const int pa = rtxu::range_first(n, d - 1, j >> 1), pcnt = rtxu::range_first(n, d - 1, (j >> 1) + 1) - pa;
    return pcnt > RTX_BUILD_LEAF_MAX ? cnt : 0;
}

// ---- triangles ----------------------------------------------------------------------------------------------------------------------------
RTX_HD bool indices_valid(int32_t i0, int32_t i1, int32_t i2, int32_t vertex_count) {
    return (uint32_t)i0 < (uint32_t)vertex_count && (uint32_t)i1 < (uint32_t)vertex_count && (uint32_t)i2 < (uint32_t)vertex_count;
}
// the centre of a valid triangle's box (halves first: the sum of two finite floats' halves is finite); false: the box is not finite
RTX_HD bool centre(const float p0[3], const float p1[3], const float p2[3], float c[3]) {
    const Box b = rtxr::triangle_box(p0, p1, p2);
    for (int a = 0; a < 3; a++) c[a] = 0.5f * b.mn[a] + 0.5f * b.mx[a];
    return rtxu::box_is_finite(b);
}
// bounds6: ordered keys of (lo.xyz, hi.xyz) over the centres of the triangles whose bit is set
RTX_HD uint64_t sort_key(const float c[3], const uint32_t bounds6[6], uint32_t index, bool valid_and_finite) {
    uint32_t code = 0;
    if (valid_and_finite)
        for (int a = 0; a < 3; a++) code |= rtxu::spread10(rtxu::cell_of(c[a], rtxu::ordered_value(bounds6[a]), rtxu::ordered_value(bounds6[3 + a]))) << (2 - a);
    return ((uint64_t)(valid_and_finite ? 1 : 0) << (RTXB_KEY_BITS - 1)) | ((uint64_t)code << RTXB_INDEX_BITS) | (uint64_t)index;
}
#define RTXB_NAN_BITS 0x7fc00000u            // every float of an invalid triangle's hot record: stored, not computed

// ---- inner nodes ----------------------------------------------------------------------------------------------------------------------------
// rtxu::join_boxes' axis (1..3) of an inner node with the stored child boxes l, r; the box itself is rtxr::join_children(l, r)
RTX_HD int join_axis(const Box & l, const Box & r) {
    float best = (r.mn[0] + r.mx[0]) - (l.mn[0] + l.mx[0]); int ax = 1;
    for (int a = 1; a < 3; a++) { const float d = (r.mn[a] + r.mx[a]) - (l.mn[a] + l.mx[a]); if (d > best) { best = d; ax = a + 1; } }
    return ax;
}

}  // namespace rtxb
