// rtx_refit.h — rtx_refit_blas on the device: a mesh's BLAS arrays rewritten in place from vertex positions in device memory, as HIP
// kernels for gfx950.  The topology stays; the arithmetic is rtx_refit_math.h, which the host twin (rtxh_blas_refit) runs too.
//
//   k_refit_triangles  one lane per flattened slot: three index loads, a gather of three vertices (and normals), whole 16-byte stores of the
//                      hot record (p0, p1 - p0, p2 - p0) and of the three normal quarters of the cold record
//   k_refit_climb      one launch for the whole bottom-up pass, whatever the depth (an SBVH chain is 40-60 levels: a launch per level would
//                      be all launch floor).  One lane per node; a leaf's lane forms the leaf box from its slots' vertices, stores it and
//                      climbs: at every parent an arrival counter decides — the first child to arrive stops, the second reads BOTH children's
//                      stored boxes, joins them left child first and goes on.  The result is a function of the input alone: which lane forms
//                      a node does not matter, what it reads is the two stored boxes.  The second arrival puts the counter back to zero, so
//                      the counters need no clearing between calls.  Nothing spins: a lane either stops or has all it needs.
//   k_refit_finish     rtxl::finish_index (rtx_layout.h): one lane per node — its packet record and six plane keys — and per 4-wide record
//                      slot — the box of the node the slot carries (slot maps made at bind), first / meta words kept
//   then rocPRIM sorts the 2 * node_count plane keys of each axis into the list plane_member (rtx_trace.h) searches.
// Every store is a vector store to an address computed from the lane's index or from tables the host filled and validated at bind
// (parents, slot maps, vertex indices in [0, vertex_count)): no index comes from the caller's float data.  A slot table written by
// rtx_build_blas (rtx_build.h) holds -1 -1 -1 for an invalid triangle: such a slot keeps a hot record of constant NaNs and is skipped in its leaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtx_device.h"
#include "rtx_refit_math.h"
#include "rtx_layout.h"

#define RTX_REFIT_BLOCK 256

struct DevRefit {
    const float *   positions;             // caller's device memory, vertex_count x 3
    const float *   normals;               // caller's device memory, vertex_count x 3, or null
    const int32_t * slot_vertices;         // tri_count x 3
    const int32_t * parent;                // node_count: parent index, -1 for the root, RTX_REFIT_UNREACHABLE
    uint32_t *      arrivals;              // node_count, zero between calls
    const int32_t * map4;                  // 2 * node_count + 4 record slots of pk4_nodes -> node, -1 = unused slot; null = binary walk
    const int32_t * map4c;                 // the same for pk4c_nodes
    float4 *        nodes;                 // the DevBlas arrays, written in place
    float4 *        pk_nodes;
    float4 *        pk4_nodes;
    float4 *        pk4c_nodes;
    float4 *        tri_hot;
    float4 *        tri_cold;              // 4 x float4 per record
    float *         plane_keys[3];         // 2 * node_count unsorted keys per axis
    int32_t         node_count, tri_count;
};

static __device__ __forceinline__ void refit_vertex(const float * __restrict__ v, const int32_t i, float out[3]) {
    out[0] = v[3 * (size_t)i]; out[1] = v[3 * (size_t)i + 1]; out[2] = v[3 * (size_t)i + 2];
}

__global__ __launch_bounds__(RTX_REFIT_BLOCK) void k_refit_triangles(const DevRefit r) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= r.tri_count) return;
    const int32_t i0 = r.slot_vertices[3 * (size_t)k], i1 = r.slot_vertices[3 * (size_t)k + 1], i2 = r.slot_vertices[3 * (size_t)k + 2];
    float v0[3], v1[3], v2[3], e1[3], e2[3];
    float4 * const hot = r.tri_hot + (size_t)RTX_TRI_STRIDE * k;                       // the fourth quarter is padding: stays
    if (i0 < 0) {                                                                      // an invalid triangle of rtx_build_blas (-1 -1 -1): stays invalid, its cold record stays
        const float q = __uint_as_float(0x7fc00000u);
        hot[0] = make_float4(q, q, q, 0.0f); hot[1] = make_float4(q, q, q, 0.0f); hot[2] = make_float4(q, q, q, 0.0f);
        return;
    }
    refit_vertex(r.positions, i0, v0); refit_vertex(r.positions, i1, v1); refit_vertex(r.positions, i2, v2);
    rtxr::edges(v0, v1, v2, e1, e2);
    hot[0] = make_float4(v0[0], v0[1], v0[2], 0.0f);
    hot[1] = make_float4(e1[0], e1[1], e1[2], 0.0f);
    hot[2] = make_float4(e2[0], e2[1], e2[2], 0.0f);
    if (r.normals) {                                                                   // rtx_triangle_cold: floats 6 .. 14 of 16
        refit_vertex(r.normals, i0, v0); refit_vertex(r.normals, i1, v1); refit_vertex(r.normals, i2, v2);
        rtxr::edges(v0, v1, v2, e1, e2);
        float4 * const cold = r.tri_cold + (size_t)4 * k;
        const float4 q1 = cold[1], q3 = cold[3];                                       // tex_coord_edge_2 and material_id ride along
        cold[1] = make_float4(q1.x, q1.y, v0[0], v0[1]);
        cold[2] = make_float4(v0[2], e1[0], e1[1], e1[2]);
        cold[3] = make_float4(e2[0], e2[1], e2[2], q3.w);
    }
}

// the box of the leaf over slots [first, first + cnt), in slot order; an invalid triangle of rtx_build_blas takes no part in any box
static __device__ __forceinline__ rtxu::Box refit_leaf_box(const DevRefit & r, const int first, const int cnt) {
    rtxu::Box b = rtxr::empty_box();
    for (int k = first; k < first + cnt; k++) {
        const int32_t i0 = r.slot_vertices[3 * (size_t)k], i1 = r.slot_vertices[3 * (size_t)k + 1], i2 = r.slot_vertices[3 * (size_t)k + 2];
        if (i0 < 0) continue;
        float v0[3], v1[3], v2[3];
        refit_vertex(r.positions, i0, v0); refit_vertex(r.positions, i1, v1); refit_vertex(r.positions, i2, v2);
        rtxr::expand_box(b, rtxr::triangle_box(v0, v1, v2));
    }
    rtxr::finish_leaf(b);
    return b;
}

__global__ __launch_bounds__(RTX_REFIT_BLOCK) void k_refit_climb(const DevRefit r) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.node_count || r.parent[i] == RTX_REFIT_UNREACHABLE) return;
    float lw = r.nodes[2 * (size_t)i].w, cw = r.nodes[2 * (size_t)i + 1].w;
    const int cnt = __float_as_int(cw) & 0x3fffffff, first = __float_as_int(lw);
    if (cnt == 0) return;                                                              // inner nodes are formed by the climb
    rtxu::Box b = refit_leaf_box(r, first, cnt);
    rtxl::store_lane(r.nodes, i, b, lw, cw);
    int cur = i;
    for (;;) {
        const int p = r.parent[cur];
        if (p < 0) return;                                                             // the root is done
        __threadfence();                                                               // this lane's box before its arrival
        if (atomicAdd(&r.arrivals[p], 1u) == 0u) return;                               // the sibling's lane will form p
        r.arrivals[p] = 0u;                                                            // nobody else looks at it in this launch
        __threadfence();                                                               // the sibling's box after its arrival
        lw = r.nodes[2 * (size_t)p].w; cw = r.nodes[2 * (size_t)p + 1].w;
        const int left = __float_as_int(lw);
        b = rtxr::join_children(rtxl::load_box(r.nodes, left), rtxl::load_box(r.nodes, left + 1));
        rtxl::store_lane(r.nodes, p, b, lw, cw);
        cur = p;
    }
}

__global__ __launch_bounds__(RTX_REFIT_BLOCK) void k_refit_finish(const DevRefit r) {
    rtxl::finish_index(r, blockIdx.x * blockDim.x + threadIdx.x, false);
}
