// rtx_update.h — rtx_update_instances on the device: the tail of Scene::update (Scene.cpp:166-170) as HIP kernels for gfx950.
//
//   instance records   one lane per instance: Mesh::update (Mesh.cpp:9-15) and the world AABB of the BLAS root box, the expressions of
//                      host/rtx_host.cpp in their order (rtx_update_math.h), so the records are the host's bit for bit
//   TLAS               the balanced tree of rtx_update_math.h: sort by (box finite?, Morton code, index), implicit heap over the sorted range, boxes
//                      bottom-up from the stored child boxes, both device node layouts (rtx_layout.h)
//
// Up to RTX_UPDATE_SMALL_MAX instances ONE workgroup does all of it in one launch (k_update_small): the scene is a few KiB, the work is a
// chain of dependent steps, and a launch costs more than any of them — bounds by LDS atomics, a bitonic sort of the 64-bit keys in LDS
// (8 KiB), the node boxes of all levels in LDS (48 KiB) with a barrier per level.  Larger scenes take one lane per element in a launch per
// step, rocPRIM's radix sort over the 47 key bits, one launch per level above level 10 and one workgroup for the levels below.
// Every store is a vector store to an address computed from the lane's own index; all indices come from n, never from the data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtx_device.h"
#include "rtx_update_math.h"
#include "rtx_layout.h"

#define RTX_UPDATE_SMALL_MAX   1024
#define RTX_UPDATE_BLOCK       1024
#define RTX_UPDATE_TOP_LEVELS  10          // levels 0 .. 10 hold at most 1024 nodes each: one workgroup, a barrier per level

struct DevUpdate {                          // the updated part of the frame state: a device block of its own (rtx_api.hip)
    const float *  positions;               // caller's device memory, n x 3
    const float *  rotations;               // caller's device memory, n x 4
    const rtx_instance * src_instances;     // where blas_id comes from (the records of the last rtx_set_frame, or this block's own)
    const DevBlas * blas;
    rtx_instance * instances;
    float *        aabbs;                   // n x 6: world AABB of every instance (min, max), before fix_if_needed
    uint32_t *     bounds;                  // 6 ordered keys: lo.xyz as they are, hi.xyz COMPLEMENTED (both reduce by min; one memset of 0xff initialises them)
    uint64_t *     keys;                    // n sort keys (after the sort: sorted)
    float4 *       nodes;                   // lane layout, 2 x float4 per slot
    float4 *       pk_nodes;                // packet layout, 2 x float4 per slot
    int32_t *      indices;
    int32_t        n, levels;
};

// Mesh::update of instance i; returns its world AABB
static __device__ __forceinline__ rtxu::Box upd_instance(const DevUpdate & u, int i, float pos[3]) {
    float rot[4];
    for (int a = 0; a < 3; a++) pos[a] = u.positions[3 * i + a];
    for (int a = 0; a < 4; a++) rot[a] = u.rotations[4 * i + a];
    const int32_t blas_id = u.src_instances[i].blas_id;
    float w[16], wi[16];
    rtxu::world_matrix(pos, rot, w);
    rtxu::invert(w, wi);
    const float4 r0 = u.blas[blas_id].nodes[0], r1 = u.blas[blas_id].nodes[1];        // root box of the uploaded BLAS (lane layout)
    const float mn[3] = { r0.x, r0.y, r0.z }, mx[3] = { r1.x, r1.y, r1.z };
    const rtxu::Box b = rtxu::transform_box(w, mn, mx);
    float4 * out = (float4 *)&u.instances[i];                                          // 144 B: blas_id + pad, world, world_inv
    *(int4 *)out = make_int4(blas_id, 0, 0, 0);
    for (int k = 0; k < 4; k++) out[1 + k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    for (int k = 0; k < 4; k++) out[5 + k] = make_float4(wi[4 * k], wi[4 * k + 1], wi[4 * k + 2], wi[4 * k + 3]);
    for (int a = 0; a < 3; a++) { u.aabbs[6 * i + a] = b.mn[a]; u.aabbs[6 * i + 3 + a] = b.mx[a]; }
    return b;
}

// Node (d, j).  LoadChild(slot) returns the stored box of a child written by level d + 1.  Returns false for a hole (zeroed).
template <typename LoadChild>
static __device__ __forceinline__ bool upd_node(const DevUpdate & u, int d, int j, rtxu::Box & b, LoadChild && load_child) {
    int first;
    const int cnt = rtxu::node_range(u.n, d, j, &first), slot = rtxu::node_slot(d, j);
    if (cnt == 0) {
        rtxl::store_hole(u.nodes, u.pk_nodes, slot);
        return false;
    }
    if (cnt == 1) {
        const int32_t inst = (int32_t)(u.keys[first] & 0xffffu);      // < n: the low key bits are the lane index the key was made from
        u.indices[first] = inst;
        for (int a = 0; a < 3; a++) { b.mn[a] = u.aabbs[6 * inst + a]; b.mx[a] = u.aabbs[6 * inst + 3 + a]; }
        rtxu::fix_if_needed(b);
        rtxl::store_node(u.nodes, u.pk_nodes, slot, b, first, 1);
        return true;
    }
    const int left = (2 << d) | (2 * j);                              // slot of (d + 1, 2j); the root's children sit at 2, 3
    int axis;
    b = rtxu::join_boxes(load_child(left), load_child(left + 1), &axis);
    rtxl::store_node(u.nodes, u.pk_nodes, slot, b, left, (int32_t)((uint32_t)axis << 30));
    return true;
}

// the six ordered-integer bounds of a wave's lanes (0xffffffff: the lane takes no part): wave64 min, then one atomic per wave and value
static __device__ __forceinline__ void upd_reduce_bounds(const uint32_t k6[6], uint32_t * bounds) {
    for (int a = 0; a < 6; a++) {
        uint32_t v = k6[a];
        for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64); v = w < v ? w : v; }
        if ((threadIdx.x & 63) == 0 && v != 0xffffffffu) atomicMin(&bounds[a], v);
    }
}

// ---- small scenes: everything in one workgroup ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(RTX_UPDATE_BLOCK) void k_update_small(const DevUpdate u) {
    __shared__ uint32_t s_bounds[6];
    __shared__ uint64_t s_keys[RTX_UPDATE_SMALL_MAX];
    __shared__ float s_box[2 * RTX_UPDATE_SMALL_MAX][6];
    const int n = u.n, tid = threadIdx.x;
    if (tid < 6) s_bounds[tid] = 0xffffffffu;
    __syncthreads();
    float pos[3] = { 0.0f, 0.0f, 0.0f };
    bool finite_box = false;
    if (tid < n) {
        finite_box = rtxu::box_is_finite(upd_instance(u, tid, pos));
        for (int a = 0; a < 3; a++) if (rtxu::is_finite(pos[a])) { const uint32_t k = rtxu::ordered_key(pos[a]); atomicMin(&s_bounds[a], k); atomicMin(&s_bounds[3 + a], ~k); }
    }
    __syncthreads();
    int P = 1; while (P < n) P <<= 1;                                  // bitonic sort over the next power of two; padding keys sort last
    if (tid < P) {
        uint64_t key = ~0ull;
        if (tid < n) { uint32_t b6[6]; rtxu::reduced_bounds(s_bounds, b6); key = rtxu::sort_key(pos, b6, (uint32_t)tid, finite_box); }
        s_keys[tid] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int other = tid ^ j;
            if (tid < P && other > tid) {
                const uint64_t a = s_keys[tid], b = s_keys[other];
                const bool up = (tid & k) == 0;
                if ((a > b) == up) { s_keys[tid] = b; s_keys[other] = a; }
            }
            __syncthreads();
        }
    if (tid < n) u.keys[tid] = s_keys[tid];
    __syncthreads();                                                   // keys and AABBs written above are read below by other lanes of this workgroup
    if (tid == 0) rtxl::store_hole(u.nodes, u.pk_nodes, 1);             // index 1: unused in the reference's arrays, zero here
    for (int d = u.levels; d >= 0; d--) {
        if (tid < (1 << d)) {
            rtxu::Box b;
            auto child = [&](int slot) { rtxu::Box c; for (int a = 0; a < 3; a++) { c.mn[a] = s_box[slot][a]; c.mx[a] = s_box[slot][3 + a]; } return c; };
            if (upd_node(u, d, tid, b, child)) { const int slot = rtxu::node_slot(d, tid); for (int a = 0; a < 3; a++) { s_box[slot][a] = b.mn[a]; s_box[slot][3 + a] = b.mx[a]; } }
        }
        __syncthreads();
    }
}

// ---- large scenes: a launch per step ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_update_instances(const DevUpdate u) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k6[6] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu };
    if (i < u.n) {
        float pos[3];
        upd_instance(u, i, pos);
        for (int a = 0; a < 3; a++) if (rtxu::is_finite(pos[a])) { const uint32_t k = rtxu::ordered_key(pos[a]); k6[a] = k; k6[3 + a] = ~k; }
    }
    upd_reduce_bounds(k6, u.bounds);
}

__global__ __launch_bounds__(256) void k_update_keys(const DevUpdate u, uint64_t * __restrict__ keys_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= u.n) return;
    uint32_t b6[6];
    rtxu::reduced_bounds(u.bounds, b6);
    const float pos[3] = { u.positions[3 * i], u.positions[3 * i + 1], u.positions[3 * i + 2] };
    rtxu::Box b;                                                       // the AABB k_update_instances stored
    for (int a = 0; a < 3; a++) { b.mn[a] = u.aabbs[6 * i + a]; b.mx[a] = u.aabbs[6 * i + 3 + a]; }
    keys_out[i] = rtxu::sort_key(pos, b6, (uint32_t)i, rtxu::box_is_finite(b));
}

// one level above RTX_UPDATE_TOP_LEVELS: children come from the lane-layout nodes the previous launch wrote
__global__ __launch_bounds__(256) void k_update_level(const DevUpdate u, const int d) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (1 << d)) return;
    rtxu::Box b;
    upd_node(u, d, j, b, [&](int slot) { return rtxl::load_box(u.nodes, slot); });
}

// levels min(levels, RTX_UPDATE_TOP_LEVELS) .. 0 in one workgroup
__global__ __launch_bounds__(RTX_UPDATE_BLOCK) void k_update_top(const DevUpdate u) {
    const int tid = threadIdx.x;
    if (tid == 0) rtxl::store_hole(u.nodes, u.pk_nodes, 1);
    for (int d = u.levels < RTX_UPDATE_TOP_LEVELS ? u.levels : RTX_UPDATE_TOP_LEVELS; d >= 0; d--) {
        if (tid < (1 << d)) {
            rtxu::Box b;
            upd_node(u, d, tid, b, [&](int slot) { return rtxl::load_box(u.nodes, slot); });
        }
        __syncthreads();                                               // the level's global stores are visible to the workgroup's next level
    }
}
