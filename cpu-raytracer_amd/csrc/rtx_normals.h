// rtx_normals.h — rtx_set_blas_topology / rtx_blas_vertex_normals on the device: smooth, area-weighted vertex normals from positions and an
// index buffer in device memory, as HIP kernels for gfx950.  The arithmetic is rtx_normals_math.h, which the host twin (rtxh_vertex_normals)
// and normals_check.cpp run too.
//
//   per topology (rtx_set_blas_topology)
//   k_normals_keys     one lane per corner c = 3 * t + k: copies the index into the library's table and writes the key (vertex << 32 | c;
//                      vertex = vertex_count for a corner of an invalid triangle)
//   then rocPRIM sorts the 3 * tri_count keys
//   k_normals_offsets  one lane per v in [0, vertex_count]: offset[v] = lower bound of v << 32 in the sorted keys — the same number of probes
//                      in every lane; no lane walks a run whose length the data decides
//   per step (rtx_blas_vertex_normals)
//   k_normals_faces    one lane per triangle: three index loads from the library's table, a gather of three vertices, ONE 16-byte store of the
//                      face vector (zeros for an invalid triangle)
//   k_normals_sum      one lane per vertex: walks sorted[offset[v] .. offset[v + 1]), loads face[c / 3] (16 bytes per incident corner), sums in
//                      ascending c, normalises, stores three dwords
// A sum per destination over stored terms, not float atomics: the order of the additions is fixed, so the bits are.  Every store is a vector
// store to an address computed from the lane's index; the only data-dependent addresses are loads — vertices through indices checked against
// [0, vertex_count) in the same lane, face vectors through corners this file's own kernels wrote (c < 3 * tri_count).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtx_normals_math.h"

#define RTX_NORMALS_BLOCK 256

struct DevNormals {
    const int32_t * indices_src;           // caller's device memory, tri_count x 3 (rtx_set_blas_topology)
    const float *   positions;             // caller's device memory, vertex_count x 3 (rtx_blas_vertex_normals)
    float *         normals_out;           // caller's device memory, vertex_count x 3
    int32_t *       indices;               // the library's copy, tri_count x 3
    uint64_t *      keys_in;               // 3 * tri_count unsorted keys
    uint64_t *      keys;                  // 3 * tri_count sorted keys
    uint32_t *      offset;                // vertex_count + 1
    float4 *        face;                  // tri_count face vectors
    int32_t         tri_count, vertex_count;
};

__global__ __launch_bounds__(RTX_NORMALS_BLOCK) void k_normals_keys(const DevNormals d) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 3u * (uint32_t)d.tri_count) return;
    const uint32_t t = c / 3u;
    const int32_t tri[3] = { d.indices_src[3 * (size_t)t], d.indices_src[3 * (size_t)t + 1], d.indices_src[3 * (size_t)t + 2] };
    d.indices[c] = tri[c - 3u * t];
    d.keys_in[c] = rtxn::corner_key(tri, c, d.vertex_count);
}

__global__ __launch_bounds__(RTX_NORMALS_BLOCK) void k_normals_offsets(const DevNormals d) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > (uint32_t)d.vertex_count) return;
    d.offset[v] = rtxn::lower_bound(d.keys, 3u * (uint32_t)d.tri_count, (uint64_t)v << 32);
}

__global__ __launch_bounds__(RTX_NORMALS_BLOCK) void k_normals_faces(const DevNormals d) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint32_t)d.tri_count) return;
    float f[3];
    rtxn::triangle_face(d.indices, d.positions, t, d.vertex_count, f);
    d.face[t] = make_float4(f[0], f[1], f[2], 0.0f);
}

__global__ __launch_bounds__(RTX_NORMALS_BLOCK) void k_normals_sum(const DevNormals d) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= (uint32_t)d.vertex_count) return;
    float n[3];
    rtxn::vertex_normal(d.keys, d.offset[v], d.offset[v + 1], d.face, n);
    float * const out = d.normals_out + 3 * (size_t)v;
    out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
}
