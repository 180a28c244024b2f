// rtx_sweep.h — swept-sphere queries (include/rtx.h: rtx_query_sweep): k_query_sweep, one kernel per round.
//
// The frame of k_query_nearest (rtx_nearest.h): one row (origin, direction, max distance, radius) per lane, RTX_QUERY_BLOCK lanes per
// workgroup, a workgroup walks one tile of RTX_QUERY_BLOCK rows to the end and fetches the next from the round's counter, so the grid never
// exceeds the threads the context's spill region was sized for.  The kernel reads the rows and writes the channels itself: no queue set, no
// resolve launch.  With an order (RTX_QUERY_SORT) slot i walks row key_row(order[i]) and scatters its answer there.
//
// The walk is rtxsp::walk (rtx_sweep_math.h), the same function the host twin runs, over the per-lane node layout and the hot triangles as
// k_query_nearest reads them.  Stack: entries (node, key), the first RTX_LDS_STACK per lane in LDS at [e][lane], deeper ones in regions 0 and 1
// of the context's spill buffer; at most rtxnp::stack_need() entries, checked on the host: no overflow path.  The cold record is read after
// the walk and only if normal, uv or material is requested (a branch on kernel arguments).  LDS: 8 KiB of staged rows + 2 x 16 KiB.
#pragma once
#include "rtx_hits.h"
#include "rtx_sweep_math.h"

// FILTERED: the masks of rtx_query_sweep_filtered (rtx_nearest.h); the stack and the tile counter are the same
template <bool FILTERED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_sweep(const DevScene sc, const float * __restrict__ rows8, const int m, const DevQuery out, const uint64_t * __restrict__ order,
                   int32_t * const spill_base, const int spill_threads, uint32_t * const head, const QueryMasks<FILTERED> masks) {
    __shared__ float lds_rows[8 * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ float lds_key[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ int lds_tile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;                  // < spill_threads: the host sizes the grid
    const size_t spill_region = (size_t)spill_threads * (RTX_MAX_STACK - RTX_LDS_STACK);
    NearestStack st = { &lds_stack[wave][0][lane], &lds_key[wave][0][lane], spill_base + gtid, (float *)(spill_base + spill_region) + gtid, spill_threads };
    const bool cold = out.normal || out.uv || out.material_id;                    // kernel arguments: the same for every lane
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    for (;;) {
        __syncthreads();                                                          // every lane has taken its row and the number of the previous tile
        if (threadIdx.x == 0) lds_tile = (int)atomicAdd(head, 1u);
        __syncthreads();
        const int tile = lds_tile;
        if (tile >= tiles) break;
        const int i = tile * RTX_QUERY_BLOCK + threadIdx.x;
        float r[8];
        if (order) query_gather_row<8>(order, rows8, m, i, r);
        else query_load_row<8>(lds_rows, rows8, m, r, tile);
        if (i >= m) continue;
        rtxsp::Answer a;
        if constexpr (FILTERED) {
            const size_t pr = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;
            Masked<HitsScene> S = { { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } }, masks.table, pr < (size_t)m ? query_row_mask(masks, pr) : 0u };
            rtxsp::walk(S, st, r, a);
        } else {
            HitsScene S = { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } };
            rtxsp::walk(S, st, r, a);
        }

        const size_t p = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;      // the caller's row of this slot
        if (p >= (size_t)m) continue;                                              // never: a sorted key holds a row of the round
        const bool hit = a.kind != rtxnp::KIND_NONE;
        rtxnp::P3 point = rtxnp::mk(0.0f, 0.0f, 0.0f), normal = point;
        float tu = 0.0f, tv = 0.0f;
        int material = -1;
        if (hit && (out.position || cold)) {
            const rtxnp::P3 q = rtxsp::centre_at(rtxnp::mk(r[0], r[1], r[2]), rtxnp::mk(r[3], r[4], r[5]), a.t);
            if (a.kind == rtxnp::KIND_TRI) nearest_triangle_outputs(sc, a.object, a.slot, a.u, a.v, out.position != nullptr, cold, point, normal, tu, tv, material);
            else if (a.kind == rtxnp::KIND_SPHERE) nearest_sphere_outputs(sc.spheres[a.object], q, point, normal, tu, tv, material);
            else nearest_plane_outputs(sc.planes[a.object], q, point, normal, tu, tv, material);
        }
        if (out.distance) out.distance[p] = hit ? a.t : INFINITY;
        if (out.position) { out.position[3 * p + 0] = point.x; out.position[3 * p + 1] = point.y; out.position[3 * p + 2] = point.z; }
        if (out.normal) { out.normal[3 * p + 0] = normal.x; out.normal[3 * p + 1] = normal.y; out.normal[3 * p + 2] = normal.z; }
        if (out.uv) { out.uv[2 * p + 0] = tu; out.uv[2 * p + 1] = tv; }
        if (out.material_id) out.material_id[p] = hit ? material : -1;
        if (out.object_id)                                            // instances, then spheres, then planes: the numbering of rtx_query_closest
            out.object_id[p] = !hit ? -1 : a.kind == rtxnp::KIND_TRI ? a.object : a.kind == rtxnp::KIND_SPHERE ? sc.instance_count + a.object : sc.instance_count + sc.sphere_count + a.object;
        if (out.triangle_id) out.triangle_id[p] = a.kind == rtxnp::KIND_TRI ? a.slot : -1;
    }
}
