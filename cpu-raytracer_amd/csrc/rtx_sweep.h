// rtx_sweep.h — swept-sphere queries (include/rtx.h: rtx_query_sweep): k_query_sweep, one kernel per round.
//
// The frame of the walk queries (rtx_nearest.h): tiles from the round's counter, the row of a slot, its caller row, the Scene (HitsScene;
// FILTERED: the masks of rtx_query_sweep_filtered), the stack of nearest_stack, the outputs of query_store_answer.  What differs:
// The row: (origin, direction, max distance, radius), eight floats.  The walk: rtxsp::walk (rtx_sweep_math.h), the function the host twin
// runs.  The distance channel is the contact's t, and the sphere and plane outputs are taken at the ball's centre there.
// LDS: 8 KiB of staged rows + 2 x 16 KiB.
#pragma once
#include "rtx_hits.h"
#include "rtx_sweep_math.h"

template <bool FILTERED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_sweep(const DevScene sc, const float * __restrict__ rows8, const int m, const DevQuery out, const uint64_t * __restrict__ order,
                   int32_t * const spill_base, const int spill_threads, uint32_t * const head, const QueryMasks<FILTERED> masks) {
    __shared__ float lds_rows[8 * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ float lds_key[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ int lds_tile;
    NearestStack st = nearest_stack(lds_stack, lds_key, spill_base, spill_threads);
    const bool cold = out.normal || out.uv || out.material_id;                    // kernel arguments: the same for every lane
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    for (;;) {
        const int tile = query_next_tile(head, lds_tile);
        if (tile >= tiles) break;
        float r[8];
        query_slot_row<8>(order, lds_rows, rows8, m, tile, r);
        size_t p;
        if (!query_caller_row(order, m, tile * RTX_QUERY_BLOCK + threadIdx.x, p)) continue;
        auto S = query_scene<HitsScene>(sc, masks, p);
        rtxsp::Answer a;
        rtxsp::walk(S, st, r, a);
        query_store_answer(sc, out, cold, p, a, [&] { return rtxsp::centre_at(rtxnp::mk(r[0], r[1], r[2]), rtxnp::mk(r[3], r[4], r[5]), a.t); }, [&] { return a.t; });
    }
}
