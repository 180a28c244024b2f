// rtx_refit_math.h — the arithmetic of the device-side mesh refit (rtx_refit_blas), written once and compiled twice like rtx_update_math.h:
// by hipcc into the kernels of rtx_refit.h and by the host compiler into rtxh_blas_refit (host/rtx_host.cpp), the specification the device
// arrays are compared with.  Unfused fp32 on both sides; only comparisons, subtractions and one addition, so the bits agree.
//
// The box rule (Device-side mesh refit):
//   triangle   AABB::from_points over its three vertices, then AABB::fix_if_needed (Triangle.h:17-22; from_points ends in a fix of its own,
//              AABB.cpp:11-22, so the fix runs twice).  A non-finite component (NaN, +-inf) is skipped: it takes no part in the min / max.
//   leaf       the union of its triangles' boxes in slot order (AABB::expand, the `a < b ? a : b` forms of Vector3::min / max); an axis on
//              which no triangle of the leaf has a finite component takes [+0, +0]; then fix_if_needed (BVHPartitions.h:11-23).
//   inner      the union of its children's STORED boxes, left child first, then fix_if_needed.
// Every stored box is therefore finite with min <= max, and a child lies inside its parent in the stored floats (min of two values is <=
// both, max is >= both, and the fix only raises max) — for every float input.  These are the preconditions of the 4-wide walks.
#pragma once
#include "rtx_update_math.h"

namespace rtxr {

using rtxu::Box;

RTX_HD Box empty_box() {                       // AABB::create_empty
    Box b;
    for (int a = 0; a < 3; a++) { b.mn[a] = INFINITY; b.mx[a] = -INFINITY; }
    return b;
}

// AABB::expand(point) on the finite components
RTX_HD void expand_point(Box & b, const float p[3]) {
    for (int a = 0; a < 3; a++) if (rtxu::is_finite(p[a])) { b.mn[a] = b.mn[a] < p[a] ? b.mn[a] : p[a]; b.mx[a] = b.mx[a] > p[a] ? b.mx[a] : p[a]; }
}

// AABB::expand(aabb): left operand first
RTX_HD void expand_box(Box & b, const Box & o) {
    for (int a = 0; a < 3; a++) { b.mn[a] = b.mn[a] < o.mn[a] ? b.mn[a] : o.mn[a]; b.mx[a] = b.mx[a] > o.mx[a] ? b.mx[a] : o.mx[a]; }
}

// Triangle::calc_aabb.  An axis without a finite component stays empty (+inf, -inf): fix_if_needed leaves it so (-inf + 0.005 = -inf)
RTX_HD Box triangle_box(const float p0[3], const float p1[3], const float p2[3]) {
    Box b = empty_box();
    expand_point(b, p0); expand_point(b, p1); expand_point(b, p2);
    rtxu::fix_if_needed(b);
    rtxu::fix_if_needed(b);
    return b;
}

// the last step of a leaf, after expand_box over its triangles' boxes in slot order
RTX_HD void finish_leaf(Box & b) {
    for (int a = 0; a < 3; a++) if (b.mn[a] > b.mx[a]) { b.mn[a] = 0.0f; b.mx[a] = 0.0f; }      // only the empty axis has min > max
    rtxu::fix_if_needed(b);
}

RTX_HD Box join_children(const Box & l, const Box & r) {
    Box b = l;
    expand_box(b, r);
    rtxu::fix_if_needed(b);
    return b;
}

// TriangleHot / the normals of TriangleCold as OBJLoader.cpp:156-175 fills them: vertex 0, and the two edges from it
RTX_HD void edges(const float v0[3], const float v1[3], const float v2[3], float e1[3], float e2[3]) {
    for (int a = 0; a < 3; a++) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; }
}

}  // namespace rtxr
