// rtx_side.h — rtx_blas_pseudonormals on the device: the angle-weighted pseudonormal tables a signed-distance query reads
// (rtx_query_signed_distance), as HIP kernels for gfx950.  The arithmetic is rtx_side_math.h, which the host twin (rtxh_blas_pseudonormals)
// and side_check.cpp run too; the inverted index (sorted corner keys, list offsets, the library's copy of the indices) is the one
// rtx_set_blas_topology built (rtx_normals.h).
//
//   per step (rtx_blas_pseudonormals), in this order on the context's stream
//   k_side_faces     one lane per SOURCE triangle: three index loads, a gather of three vertices, FOUR 16-byte stores — the unit normal and
//                    the three angle-weighted corner vectors (RTX_SIDE_RECORD float4 per triangle; zeros for an invalid triangle)
//   k_side_vertices  one lane per vertex: walks sorted[offset[v] .. offset[v + 1]), loads the corner vector of every incident corner (16 bytes,
//                    four loads in flight), sums in ascending c, ONE 16-byte store
//   k_side_edges     one lane per (slot, edge): the edge's two vertices from slot_vertices, then the list of the first, the unit normal of
//                    every listed triangle that also holds the second (its three indices and its record, two triangles in flight), summed in
//                    ascending c, ONE 16-byte store — so a query lane's lookup is a single 16-byte load
// Sums per destination over stored terms, not float atomics: the order of the additions is fixed, so the bits are.  No LDS, no atomics.  Every
// store is a vector store to an address computed from the lane's index; the only data-dependent addresses are loads — vertices through
// indices checked against [0, vertex_count) in the same lane, records through corners of the inverted index (c < 3 * tri_count), lists
// through slot vertices checked against [0, vertex_count) in the same lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtx_normals.h"
#include "rtx_side_math.h"

#define RTX_SIDE_BLOCK 256

struct DevSide {
    const float *    positions;             // caller's device memory, vertex_count x 3 (rtx_blas_pseudonormals)
    const int32_t *  indices;               // the topology's copy of the indices, tri_count x 3 (DevNormals::indices)
    const uint64_t * keys;                  // 3 * tri_count sorted corner keys (DevNormals::keys)
    const uint32_t * offset;                // vertex_count + 1 (DevNormals::offset)
    const int32_t *  slot_vertices;         // the BLAS's slot -> vertex table, slots x 3 (DevRefit::slot_vertices)
    float4 *         record;                // RTX_SIDE_RECORD x tri_count
    float4 *         vert_pn;               // vertex_count
    float4 *         edge_pn;               // 3 x slots
    int32_t          tri_count, vertex_count, slots;
};

// what a SIGNED query reads of one BLAS id (an array with one entry per id, beside the DevBlas table and not in it); all null: no tables
struct DevSideBlas { const float4 * vert_pn; const float4 * edge_pn; const int32_t * slot_vertices; int32_t vertex_count, pad; };

__global__ __launch_bounds__(RTX_SIDE_BLOCK) void k_side_faces(const DevSide d) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint32_t)d.tri_count) return;
    float rec[16];
    rtxsd::triangle_record(d.indices, d.positions, t, d.vertex_count, rec);
    float4 * const out = d.record + RTX_SIDE_RECORD * (size_t)t;
    out[0] = make_float4(rec[0], rec[1], rec[2], rec[3]);
    out[1] = make_float4(rec[4], rec[5], rec[6], rec[7]);
    out[2] = make_float4(rec[8], rec[9], rec[10], rec[11]);
    out[3] = make_float4(rec[12], rec[13], rec[14], rec[15]);
}

__global__ __launch_bounds__(RTX_SIDE_BLOCK) void k_side_vertices(const DevSide d) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (uint32_t)d.vertex_count) return;
    float n[4];
    rtxsd::vertex_pseudonormal(d.keys, d.offset[v], d.offset[v + 1], (const float4 *)d.record, n);
    d.vert_pn[v] = make_float4(n[0], n[1], n[2], n[3]);
}

__global__ __launch_bounds__(RTX_SIDE_BLOCK) void k_side_edges(const DevSide d) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3u * (uint32_t)d.slots) return;
    const uint32_t s = e / 3u;
    const int32_t sv[3] = { d.slot_vertices[3 * (size_t)s], d.slot_vertices[3 * (size_t)s + 1], d.slot_vertices[3 * (size_t)s + 2] };
    int32_t x, y;
    rtxsd::edge_vertices(sv, (int)(e - 3u * s), x, y);
    float n[4];
    rtxsd::edge_pseudonormal(d.keys, d.offset, d.indices, (const float4 *)d.record, d.vertex_count, x, y, n);
    d.edge_pn[e] = make_float4(n[0], n[1], n[2], n[3]);
}
