// rtx_overlap.h — box-overlap queries (include/rtx.h: rtx_query_overlap): k_query_overlap, one kernel per round.
//
// The frame of the walk queries (rtx_nearest.h): tiles from the round's counter (query_next_tile); the row of a slot, its caller row and the
// Scene (FILTERED: the masks of rtx_query_overlap_filtered) are spelled out in the kernel and must match the frame's functions.  What differs:
// The row: (centre, half extents, quaternion), ten floats.  The walk: rtxop::walk (rtx_overlap_math.h), the function the host twin runs.
// The kernel writes the ids of the K smallest overlaps of every row and the row's count.
// Stack: node ids only (the walk has no key: nothing is tested again when popped), the first RTX_LDS_STACK per lane in LDS at [e][lane],
// deeper ones in region 0 of the context's spill buffer; the host's stack rule is the same.
// The list: (object, triangle) per held overlap, two dwords, in LDS at [entry][field][lane] — one dword per lane and
// instruction, conflict free like the stack, and addressed by a runtime entry without a private array (which would live in scratch).
// The lane's row stays in LDS during the walk (a sorted round writes the gathered row there too): the walk holds ONE frame and makes the
// world frame again from the row when an instance is done (holding both frames in registers measured no better: DESIGN.md 3).
// FORM: the walk's form (rtxop::FORM_*), plus OVERLAP_COUNT_ONLY for the listing forms without a list; ANY never has one.
// LDS: 10 KiB of staged rows + 16 KiB of stack + 16 KiB of list (the listing forms) = 42 KiB, 26 KiB without a list.
#pragma once
#include "rtx_nearest.h"
#include "rtx_overlap_math.h"

enum { OVERLAP_COUNT_ONLY = 4 };                  // a bit of k_query_overlap's FORM beside rtxop::FORM_TRIANGLES / FORM_OBJECTS

struct OverlapScene : NearestScene {
    RTX_D int instance_count() const { return sc.instance_count; }
    RTX_D int enter(int slot, rtxop::Frame & F) {
        const int inst = sc.tlas_indices[slot];
        const rtx_instance & I = sc.instances[inst];
        F = rtxop::local_frame(F, I.world_inv);
        const DevBlas & B = sc.blas[I.blas_id];
        nodes = RTX_GPTR(B.nodes); tris = RTX_GPTR(B.tri_hot);
        return inst;
    }
};

struct OverlapStack {             // entry sp of this lane: LDS at stk[sp * RTX_WAVE], then region 0 of the spill buffer
    int * stk; int * spill; int stride;
    RTX_D void push(int sp, int node) {
        if (sp < RTX_LDS_STACK) stk[sp * RTX_WAVE] = node;
        else spill[(sp - RTX_LDS_STACK) * stride] = node;
    }
    RTX_D void pop(int sp, int & node) const {
        if (sp < RTX_LDS_STACK) node = stk[sp * RTX_WAVE];
        else node = spill[(sp - RTX_LDS_STACK) * stride];
    }
};

struct OverlapList {              // entry j of this lane: fields at base[(2 * j + f) * RTX_QUERY_BLOCK]
    int32_t * base;
    RTX_D void get(int j, int32_t & object, int32_t & triangle) const {
        const int32_t * const p = base + 2 * j * RTX_QUERY_BLOCK;
        object = p[0]; triangle = p[RTX_QUERY_BLOCK];
    }
    RTX_D void set(int j, int32_t object, int32_t triangle) {
        int32_t * const p = base + 2 * j * RTX_QUERY_BLOCK;
        p[0] = object; p[RTX_QUERY_BLOCK] = triangle;
    }
};
struct OverlapNoList {            // ANY and the count-only forms: offer() returns before it touches a list
    RTX_D void get(int, int32_t & object, int32_t & triangle) const { object = -1; triangle = -1; }
    RTX_D void set(int, int32_t, int32_t) {}
};

// rows10: the m boxes of the round; object_id, triangle_id: the caller's arrays advanced to the round's first row (K entries per row), or
// null; count: likewise ([m]; 0 / 1 in the ANY form), or null
template <int FORM, bool FILTERED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_overlap(const DevScene sc, const float * __restrict__ rows10, const int m, const int K, int32_t * __restrict__ object_id, int32_t * __restrict__ triangle_id,
                     int32_t * __restrict__ count, const uint64_t * __restrict__ order, int32_t * const spill_base, const int spill_threads, uint32_t * const head,
                     const QueryMasks<FILTERED> masks) {
    constexpr int WALK = FORM & 3;
    constexpr bool LIST = WALK != rtxop::FORM_ANY && !(FORM & OVERLAP_COUNT_ONLY);
    __shared__ float lds_rows[rtxop::ROW_FLOATS * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ int32_t lds_list[LIST ? 2 * rtxop::MAX_HITS * RTX_QUERY_BLOCK : 1];
    __shared__ int lds_tile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;                  // < spill_threads: the host sizes the grid
    OverlapStack st = { &lds_stack[wave][0][lane], spill_base + gtid, spill_threads };
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    for (;;) {
        const int tile = query_next_tile(head, lds_tile);
        if (tile >= tiles) break;
        const int i = tile * RTX_QUERY_BLOCK + threadIdx.x;
        float r[rtxop::ROW_FLOATS];
        float * const row = &lds_rows[threadIdx.x * rtxop::ROW_FLOATS];          // the lane's row stays in LDS for the walk, which reads it again
        // From here to the caller row: query_slot_row, query_caller_row and query_scene spelled out; they must match those functions
        // (rtx_nearest.h's header comment says why)
        if (order) { query_gather_row<rtxop::ROW_FLOATS>(order, rows10, m, i, r); for (int k = 0; k < rtxop::ROW_FLOATS; k++) row[k] = r[k]; }
        else query_load_row<rtxop::ROW_FLOATS>(lds_rows, rows10, m, r, tile);
        if (i >= m) continue;
        rtxop::Tally w;
        typename std::conditional<LIST, OverlapList, OverlapNoList>::type L;
        if constexpr (LIST) L.base = &lds_list[threadIdx.x];
        if constexpr (FILTERED) {
            const size_t pr = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;
            Masked<OverlapScene> S = { { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } }, masks.table, pr < (size_t)m ? query_row_mask(masks, pr) : 0u };
            rtxop::walk<WALK>(S, st, L, row, LIST ? K : 0, w);
        } else {
            OverlapScene S = { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } };
            rtxop::walk<WALK>(S, st, L, row, LIST ? K : 0, w);
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
