// rtx_boxsweep.h — swept-box queries (include/rtx.h: rtx_query_sweep_box): k_query_sweep_box, one kernel per round.
//
// The frame of the walk queries (rtx_nearest.h): tiles from the round's counter, the row of a slot, its caller row, the Scene (FILTERED: the
// masks of rtx_query_sweep_box_filtered), the stack of nearest_stack (entries (node, key), LDS at [e][lane], spill regions 0 and 1).  What
// differs:
// The row: (centre, direction, max distance, half extents, quaternion), fourteen floats.  The walk: rtxbs::walk (rtx_boxsweep_math.h), the
// function the host twin runs.  The lane's row stays in LDS during the walk, as in k_query_overlap (a sorted round writes the gathered row
// there too): the walk holds ONE frame and makes the world frame, direction and velocity again from the row when an instance is done.
// The outputs: t, the contact normal, the ids and the axis code, each its own array.  The normal is computed after the walk from the winner
// alone and only if requested (a branch on a kernel argument): the instance's matrix and two 16-byte hot loads for a triangle.
// LDS: 14 KiB of staged rows + 2 x 16 KiB.
#pragma once
#include "rtx_overlap.h"
#include "rtx_boxsweep_math.h"

struct BoxSweepScene : NearestScene {
    RTX_D int instance_count() const { return sc.instance_count; }
    RTX_D int enter(int slot, rtxop::Frame & F, rtxnp::P3 & cd) {
        const int inst = sc.tlas_indices[slot];
        const rtx_instance & I = sc.instances[inst];
        F = rtxop::local_frame(F, I.world_inv);
        cd = rtxnp::xform_dir(I.world_inv, cd);
        const DevBlas & B = sc.blas[I.blas_id];
        nodes = RTX_GPTR(B.nodes); tris = RTX_GPTR(B.tri_hot);
        return inst;
    }
};

// the output arrays of one round, advanced to its first row; null = not requested
struct DevBoxSweep { float * t; float * normal; int32_t * object_id; int32_t * triangle_id; int32_t * axis; };

// NORMAL of rtx_boxsweep_math.h for the answer a of the row
RTX_D rtxnp::P3 boxsweep_normal(const DevScene & sc, const float * row, const rtxbs::Answer & a) {
    if (a.object < 0 || a.t == 0.0f) return rtxnp::mk(0.0f, 0.0f, 0.0f);
    const rtxop::Frame W = rtxbs::world_frame(row);
    const rtxnp::P3 d = rtxnp::mk(row[3], row[4], row[5]);
    if (a.slot >= 0) {
        const rtx_instance & I = sc.instances[a.object];
        const rtx_gptr hp = RTX_GPTR(sc.blas[I.blas_id].tri_hot);
        const float4 e1 = gld(hp, RTX_TRI_STRIDE * a.slot + 1), e2 = gld(hp, RTX_TRI_STRIDE * a.slot + 2);
        return rtxbs::triangle_normal(W, I.world_inv, rtxnp::mk(e1.x, e1.y, e1.z), rtxnp::mk(e2.x, e2.y, e2.z), a.axis, d);
    }
    if (a.axis == rtxbs::AXIS_SPHERE) { const rtx_sphere & s = sc.spheres[a.object - sc.instance_count]; return rtxbs::sphere_normal(W, d, rtxnp::ptr3(s.center), s.radius_squared, a.t); }
    const rtx_plane & pl = sc.planes[a.object - sc.instance_count - sc.sphere_count];
    return rtxbs::plane_normal(W, rtxnp::ptr3(pl.normal), pl.distance);
}

template <bool FILTERED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_sweep_box(const DevScene sc, const float * __restrict__ rows14, const int m, const DevBoxSweep out, const uint64_t * __restrict__ order,
                       int32_t * const spill_base, const int spill_threads, uint32_t * const head, const QueryMasks<FILTERED> masks) {
    __shared__ float lds_rows[rtxbs::ROW_FLOATS * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ float lds_key[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ int lds_tile;
    NearestStack st = nearest_stack(lds_stack, lds_key, spill_base, spill_threads);
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    for (;;) {
        const int tile = query_next_tile(head, lds_tile);
        if (tile >= tiles) break;
        float r[rtxbs::ROW_FLOATS];
        float * const row = &lds_rows[threadIdx.x * rtxbs::ROW_FLOATS];          // the lane's row stays in LDS for the walk, which reads it again
        query_slot_row<rtxbs::ROW_FLOATS>(order, lds_rows, rows14, m, tile, r);
        if (order) for (int k = 0; k < rtxbs::ROW_FLOATS; k++) row[k] = r[k];    // a sorted round: the gathered row, into the lane's own slot
        size_t p;
        if (!query_caller_row(order, m, tile * RTX_QUERY_BLOCK + threadIdx.x, p)) continue;
        auto S = query_scene<BoxSweepScene>(sc, masks, p);
        rtxbs::Answer a;
        rtxbs::walk(S, st, row, a);
        if (out.t) out.t[p] = a.t;
        if (out.normal) {
            const rtxnp::P3 n = boxsweep_normal(sc, row, a);
            out.normal[3 * p + 0] = n.x; out.normal[3 * p + 1] = n.y; out.normal[3 * p + 2] = n.z;
        }
        if (out.object_id) out.object_id[p] = a.object;
        if (out.triangle_id) out.triangle_id[p] = a.slot;
        if (out.axis) out.axis[p] = a.axis;
    }
}
