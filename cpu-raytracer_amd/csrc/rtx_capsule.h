// rtx_capsule.h — capsule-overlap queries (include/rtx.h: rtx_query_overlap_capsule): k_query_overlap_capsule, one kernel per round.
//
// The shape of k_query_overlap (rtx_overlap.h), whose stack (OverlapStack: node ids, the first RTX_LDS_STACK per lane in LDS, deeper ones in
// region 0 of the spill buffer), lists (OverlapList / OverlapNoList) and FORM bits it uses.  What differs:
// The row: (start point, axis vector, radius), seven floats; with an order (RTX_QUERY_SORT) the ray key over the first six.  The walk:
// rtxcp::walk (rtx_capsule_math.h), the function the host twin runs.
// The lane's row stays in LDS during the walk at stride 7 — odd, so the 64 lanes of a wave read 64 different banks — and the walk holds ONE
// frame: the world frame is read again from the row when an instance is done.
// LDS: 7 KiB of staged rows + 16 KiB of stack + 16 KiB of list (the listing forms) = 39 KiB, 23 KiB without a list.
#pragma once
#include "rtx_overlap.h"
#include "rtx_capsule_math.h"

struct CapsuleScene : NearestScene {
    RTX_D int instance_count() const { return sc.instance_count; }
    RTX_D int enter(int slot, rtxcp::Frame & F) {
        const int inst = sc.tlas_indices[slot];
        const rtx_instance & I = sc.instances[inst];
        F = rtxcp::local_frame(F, I.world_inv);
        const DevBlas & B = sc.blas[I.blas_id];
        nodes = RTX_GPTR(B.nodes); tris = RTX_GPTR(B.tri_hot);
        return inst;
    }
};

// rows7: the m capsules of the round; object_id, triangle_id: the caller's arrays advanced to the round's first row (K entries per row), or
// null; count: likewise ([m]; 0 / 1 in the ANY form), or null
template <int FORM, bool FILTERED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_overlap_capsule(const DevScene sc, const float * __restrict__ rows7, const int m, const int K, int32_t * __restrict__ object_id, int32_t * __restrict__ triangle_id,
                             int32_t * __restrict__ count, const uint64_t * __restrict__ order, int32_t * const spill_base, const int spill_threads, uint32_t * const head,
                             const QueryMasks<FILTERED> masks) {
    constexpr int WALK = FORM & 3;
    constexpr bool LIST = WALK != rtxcp::FORM_ANY && !(FORM & OVERLAP_COUNT_ONLY);
    __shared__ float lds_rows[rtxcp::ROW_FLOATS * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ int32_t lds_list[LIST ? 2 * rtxcp::MAX_HITS * RTX_QUERY_BLOCK : 1];
    __shared__ int lds_tile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;                  // < spill_threads: the host sizes the grid
    OverlapStack st = { &lds_stack[wave][0][lane], spill_base + gtid, spill_threads };
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    for (;;) {
        const int tile = query_next_tile(head, lds_tile);
        if (tile >= tiles) break;
        const int i = tile * RTX_QUERY_BLOCK + threadIdx.x;
        float r[rtxcp::ROW_FLOATS];
        float * const row = &lds_rows[threadIdx.x * rtxcp::ROW_FLOATS];          // the lane's row stays in LDS for the walk, which reads it again
        // From here to the caller row: query_slot_row, query_caller_row and query_scene spelled out as in k_query_overlap; they must match
        // those functions (rtx_nearest.h's header comment says why)
        if (order) { query_gather_row<rtxcp::ROW_FLOATS>(order, rows7, m, i, r); for (int k = 0; k < rtxcp::ROW_FLOATS; k++) row[k] = r[k]; }
        else query_load_row<rtxcp::ROW_FLOATS>(lds_rows, rows7, m, r, tile);
        if (i >= m) continue;
        rtxop::Tally w;
        typename std::conditional<LIST, OverlapList, OverlapNoList>::type L;
        if constexpr (LIST) L.base = &lds_list[threadIdx.x];
        if constexpr (FILTERED) {
            const size_t pr = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;
            Masked<CapsuleScene> S = { { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } }, masks.table, pr < (size_t)m ? query_row_mask(masks, pr) : 0u };
            rtxcp::walk<WALK>(S, st, L, row, LIST ? K : 0, w);
        } else {
            CapsuleScene S = { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } };
            rtxcp::walk<WALK>(S, st, L, row, LIST ? K : 0, w);
        }
        const size_t p = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;      // the caller's row of this slot
        if (p >= (size_t)m) continue;                                              // never: a sorted key holds a row of the round
        if (count) count[p] = w.count;
        if constexpr (LIST) {
            for (int j = 0; j < K; j++) {
                const size_t e = p * (size_t)K + (size_t)j;
                int32_t object = -1, triangle = -1;
                if (j < w.held) L.get(j, object, triangle);
                if (object_id) object_id[e] = object;
                if (triangle_id) triangle_id[e] = triangle;
            }
        }
    }
}
