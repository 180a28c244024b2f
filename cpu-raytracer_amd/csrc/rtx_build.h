// rtx_build.h — rtx_build_blas on the device: a mesh's BLAS built from triangles (positions + indices) in device memory, as HIP kernels
// for gfx950.  The tree is the balanced one of rtx_build_math.h, whose topology rtx_alloc_blas computed from the triangle count and uploaded
// with the refit plan (rtx_refit.h: parents, slot maps); a build sorts the triangles into it and writes triangles, boxes and axis bits.
//
//   k_build_bounds   one lane per source triangle: index check, centre of its box, wave64 shuffle reduction of the six ordered-integer
//                    bounds, one atomicMin per wave and bound
//   k_build_keys     one lane per source triangle: the 55-bit sort key
//   rocPRIM          radix sort of the keys over the used bits
//   k_build_scatter  one lane per sorted slot: the slot table (three vertex indices, or -1 -1 -1 for an invalid triangle), the hot and cold
//                    records in whole 16-byte stores, order_out
//   k_build_level    one launch per level below RTX_BUILD_TOP_LEVELS, one lane per node of the level: a leaf's box from its slots, an inner
//                    node's from its children's STORED boxes with the axis into bits 30-31 of `count`
//   k_build_top      levels RTX_BUILD_TOP_LEVELS .. 0 in one workgroup, a barrier per level (the heap is regular: no arrival counters)
//   k_build_finish   k_refit_finish's pass (rtxl::finish_index, rtx_layout.h) with the axis fields of the pk4c meta words composed anew
//   then the three plane sorts of the refit.
// Indices come from the caller's device memory here: every one is checked against [0, vertex_count) before it is used as an address, in
// every kernel that reads it.  All other addresses come from the lane's index, the alloc-time tables or the keys this file made.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtx_device.h"
#include "rtx_refit.h"
#include "rtx_update.h"                      // upd_reduce_bounds
#include "rtx_build_math.h"

#define RTX_BUILD_BLOCK       256
#define RTX_BUILD_TOP_BLOCK   1024
#define RTX_BUILD_TOP_LEVELS  10           // levels 0 .. 10 hold at most 1024 nodes each

struct DevBuild {
    const float *   positions;             // caller's device memory, vertex_count x 3
    const int32_t * indices;               // caller's device memory, tri_count x 3
    const float *   normals;               // caller's device memory, vertex_count x 3
    const float *   texcoords;             // caller's device memory, vertex_count x 2, or null: zeros
    int32_t *       order_out;             // caller's device memory, tri_count, or null
    const int32_t * material_ids;          // tri_count local ids per SOURCE triangle (alloc-time table, validated on the host)
    uint32_t *      bounds;                // 6 ordered keys: lo.xyz as they are, hi.xyz COMPLEMENTED (both reduce by min; one memset of 0xff initialises them)
    uint64_t *      keys_in;               // tri_count unsorted keys
    uint64_t *      keys;                  // tri_count sorted keys
    int32_t *       slot_vertices;         // tri_count x 3: the refit's slot table, written per build
    int32_t         tri_count, vertex_count;
};

// source triangle t: true when its indices are valid and its box is finite; c = the centre of the box then
static __device__ __forceinline__ bool build_centre(const DevBuild & b, const int t, float c[3]) {
    const int32_t i0 = b.indices[3 * (size_t)t], i1 = b.indices[3 * (size_t)t + 1], i2 = b.indices[3 * (size_t)t + 2];
    if (!rtxb::indices_valid(i0, i1, i2, b.vertex_count)) return false;
    float v0[3], v1[3], v2[3];
    refit_vertex(b.positions, i0, v0); refit_vertex(b.positions, i1, v1); refit_vertex(b.positions, i2, v2);
    return rtxb::centre(v0, v1, v2, c);
}

__global__ __launch_bounds__(RTX_BUILD_BLOCK) void k_build_bounds(const DevBuild b) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k6[6] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu };
    float c[3];
    if (t < b.tri_count && build_centre(b, t, c))
        for (int a = 0; a < 3; a++) { const uint32_t k = rtxu::ordered_key(c[a]); k6[a] = k; k6[3 + a] = ~k; }
    upd_reduce_bounds(k6, b.bounds);
}

__global__ __launch_bounds__(RTX_BUILD_BLOCK) void k_build_keys(const DevBuild b) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b.tri_count) return;
    uint32_t b6[6];
    rtxu::reduced_bounds(b.bounds, b6);
    float c[3] = { 0.0f, 0.0f, 0.0f };
    const bool ok = build_centre(b, t, c);
    b.keys_in[t] = rtxb::sort_key(c, b6, (uint32_t)t, ok);
}

__global__ __launch_bounds__(RTX_BUILD_BLOCK) void k_build_scatter(const DevBuild b, const DevRefit r) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.tri_count) return;
    int t = (int)(b.keys[k] & (((uint64_t)1 << RTXB_INDEX_BITS) - 1));            // the lane index k_build_keys made the key from
    if (t >= b.tri_count) t = k;                                                       // never true for keys this file made; no address depends on trusting them
    const int32_t i0 = b.indices[3 * (size_t)t], i1 = b.indices[3 * (size_t)t + 1], i2 = b.indices[3 * (size_t)t + 2];
    const bool valid = rtxb::indices_valid(i0, i1, i2, b.vertex_count);
    b.slot_vertices[3 * (size_t)k]     = valid ? i0 : -1;
    b.slot_vertices[3 * (size_t)k + 1] = valid ? i1 : -1;
    b.slot_vertices[3 * (size_t)k + 2] = valid ? i2 : -1;
    if (b.order_out) b.order_out[k] = t;
    float4 * const hot = r.tri_hot + (size_t)RTX_TRI_STRIDE * k;                       // the fourth quarter is padding: stays zero
    float4 * const cold = r.tri_cold + (size_t)4 * k;
    const float mat = __int_as_float(b.material_ids[t]);
    if (!valid) {
        const float q = __uint_as_float(RTXB_NAN_BITS);
        hot[0] = make_float4(q, q, q, 0.0f); hot[1] = make_float4(q, q, q, 0.0f); hot[2] = make_float4(q, q, q, 0.0f);
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        cold[0] = z; cold[1] = z; cold[2] = z; cold[3] = make_float4(0.0f, 0.0f, 0.0f, mat);
        return;
    }
    float v0[3], v1[3], v2[3], e1[3], e2[3];
    refit_vertex(b.positions, i0, v0); refit_vertex(b.positions, i1, v1); refit_vertex(b.positions, i2, v2);
    rtxr::edges(v0, v1, v2, e1, e2);
    hot[0] = make_float4(v0[0], v0[1], v0[2], 0.0f);
    hot[1] = make_float4(e1[0], e1[1], e1[2], 0.0f);
    hot[2] = make_float4(e2[0], e2[1], e2[2], 0.0f);
    float t0[2] = { 0.0f, 0.0f }, u1[2] = { 0.0f, 0.0f }, u2[2] = { 0.0f, 0.0f };
    if (b.texcoords) {
        const float * const uv = b.texcoords;
        t0[0] = uv[2 * (size_t)i0]; t0[1] = uv[2 * (size_t)i0 + 1];
        u1[0] = uv[2 * (size_t)i1] - t0[0]; u1[1] = uv[2 * (size_t)i1 + 1] - t0[1];
        u2[0] = uv[2 * (size_t)i2] - t0[0]; u2[1] = uv[2 * (size_t)i2 + 1] - t0[1];
    }
    refit_vertex(b.normals, i0, v0); refit_vertex(b.normals, i1, v1); refit_vertex(b.normals, i2, v2);
    rtxr::edges(v0, v1, v2, e1, e2);
    cold[0] = make_float4(t0[0], t0[1], u1[0], u1[1]);                                 // rtx_triangle_cold, 16 floats
    cold[1] = make_float4(u2[0], u2[1], v0[0], v0[1]);
    cold[2] = make_float4(v0[2], e1[0], e1[1], e1[2]);
    cold[3] = make_float4(e2[0], e2[1], e2[2], mat);
}

// node i of the alloc-time topology: a leaf's box from its slots (invalid slots skipped), an inner node's from its children's stored boxes
static __device__ __forceinline__ void build_node(const DevRefit & r, const int i) {
    if (r.parent[i] == RTX_REFIT_UNREACHABLE) return;                                  // holes and index 1 stay zero
    const float lw = r.nodes[2 * (size_t)i].w, cw = r.nodes[2 * (size_t)i + 1].w;
    const int cnt = __float_as_int(cw) & 0x3fffffff, first = __float_as_int(lw);
    if (cnt > 0) { rtxl::store_lane(r.nodes, i, refit_leaf_box(r, first, cnt), lw, cw); return; }
    const int left = first;
    const rtxu::Box l = rtxl::load_box(r.nodes, left), rr = rtxl::load_box(r.nodes, left + 1);
    rtxl::store_lane(r.nodes, i, rtxr::join_children(l, rr), lw, __int_as_float((int32_t)((uint32_t)rtxb::join_axis(l, rr) << 30)));
}

// level d > RTX_BUILD_TOP_LEVELS: nodes 2^d .. 2^(d+1) - 1; the children come from the launch before
__global__ __launch_bounds__(RTX_BUILD_BLOCK) void k_build_level(const DevRefit r, const int d) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < (1 << d)) build_node(r, (1 << d) + j);
}

// levels min(levels, RTX_BUILD_TOP_LEVELS) .. 0 in one workgroup
__global__ __launch_bounds__(RTX_BUILD_TOP_BLOCK) void k_build_top(const DevRefit r, const int levels) {
    const int tid = threadIdx.x;
    for (int d = levels < RTX_BUILD_TOP_LEVELS ? levels : RTX_BUILD_TOP_LEVELS; d >= 0; d--) {
        if (tid < (1 << d)) build_node(r, rtxu::node_slot(d, tid));
        __syncthreads();                                               // the level's global stores are visible to the workgroup's next level
    }
}

// k_refit_finish's pass, and the axis fields of the pk4c meta words from the count words the levels above have written
__global__ __launch_bounds__(RTX_REFIT_BLOCK) void k_build_finish(const DevRefit r) {
    rtxl::finish_index(r, blockIdx.x * blockDim.x + threadIdx.x, true);
}
