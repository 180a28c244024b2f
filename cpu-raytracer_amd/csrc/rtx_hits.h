// rtx_hits.h — all-hits segment queries (include/rtx.h: rtx_query_hits): k_query_hits, one kernel per round.
//
// The frame of the walk queries (rtx_nearest.h): tiles from the round's counter, the row of a slot, its caller row, the Scene (FILTERED: the
// masks of rtx_query_hits_filtered), the stack of nearest_stack, the channel stores.  What differs:
// The row: (origin, direction, max distance), seven floats.  The walk: rtxhp::walk (rtx_hits_math.h), the function the host twin runs.
// The kernel writes the channels of the first K hits of every row, in order, and the row's count.
// The list: (t, object, triangle) per held hit, three dwords, in LDS at [entry][field][lane] — one dword per lane and instruction, conflict
// free like the stack, and addressed by a runtime entry without a private array (which would live in scratch).  u and v are not kept: after
// the walk tri_test runs again on the at most K listed triangles, then the requested channels are rebuilt; the cold record is read only if
// normal, uv or material is requested (a branch on kernel arguments).  LIST = false is the count-only form: no list, one register.
// LDS: 7 KiB of staged rows + 2 x 16 KiB of stack + 24 KiB of list = 63 KiB, two workgroups per CU.
#pragma once
#include "rtx_nearest.h"
#include "rtx_hits_math.h"

struct HitsScene : NearestScene {
    RTX_D int instance_count() const { return sc.instance_count; }
    RTX_D int enter(int slot, rtxnp::P3 o, rtxnp::P3 d, rtxnp::P3 & co, rtxnp::P3 & cd) {
        const int inst = sc.tlas_indices[slot];
        const rtx_instance & I = sc.instances[inst];
        co = rtxnp::xform_pos(I.world_inv, o);
        cd = rtxnp::xform_dir(I.world_inv, d);
        const DevBlas & B = sc.blas[I.blas_id];
        nodes = RTX_GPTR(B.nodes); tris = RTX_GPTR(B.tri_hot);
        return inst;
    }
};

struct HitsList {                 // entry j of this lane: fields at base[(3 * j + f) * RTX_QUERY_BLOCK]
    float * base;
    RTX_D void get(int j, float & t, int32_t & object, int32_t & triangle) const {
        const float * const p = base + 3 * j * RTX_QUERY_BLOCK;
        t = p[0]; object = as_i(p[RTX_QUERY_BLOCK]); triangle = as_i(p[2 * RTX_QUERY_BLOCK]);
    }
    RTX_D void set(int j, float t, int32_t object, int32_t triangle) {
        float * const p = base + 3 * j * RTX_QUERY_BLOCK;
        p[0] = t; p[RTX_QUERY_BLOCK] = as_f(object); p[2 * RTX_QUERY_BLOCK] = as_f(triangle);
    }
};
struct HitsNoList {               // the count-only form: offer() returns before it touches a list
    RTX_D void get(int, float & t, int32_t & object, int32_t & triangle) const { t = 0.0f; object = -1; triangle = -1; }
    RTX_D void set(int, float, int32_t, int32_t) {}
};

// the channels of hit (t, object, triangle) of the row (o, d): element e of every requested channel
RTX_D void hit_write(const DevScene & sc, const DevQuery & out, const bool cold, const size_t e, const rtxnp::P3 o, const rtxnp::P3 d, const float D,
                     const float t, const int32_t object, const int32_t triangle) {
    rtxnp::P3 point = rtxnp::mk(0.0f, 0.0f, 0.0f), normal = point;
    float tu = 0.0f, tv = 0.0f;
    int material = -1;
    if (out.position || cold) {
        if (triangle >= 0) {
            const rtx_instance & I = sc.instances[object];
            const DevBlas & B = sc.blas[I.blas_id];
            const rtxnp::P3 co = rtxnp::xform_pos(I.world_inv, o), cd = rtxnp::xform_dir(I.world_inv, d);
            point = rtxnp::xform_pos(I.world, rtxhp::point_at(co, cd, t));
            if (cold) {
                float u = 0.0f, v = 0.0f;
                if (out.normal || out.uv) {
                    const rtx_gptr hp = RTX_GPTR(B.tri_hot);
                    const float4 p0 = gld(hp, RTX_TRI_STRIDE * triangle), e1 = gld(hp, RTX_TRI_STRIDE * triangle + 1), e2 = gld(hp, RTX_TRI_STRIDE * triangle + 2);
                    float t2;
                    rtxhp::tri_test(rtxnp::mk(p0.x, p0.y, p0.z), rtxnp::mk(e1.x, e1.y, e1.z), rtxnp::mk(e2.x, e2.y, e2.z), co, cd, D, t2, u, v);
                }
                const rtx_gptr cp = RTX_GPTR(B.tri_cold + triangle);                 // 64-byte record = 4 x dwordx4, fields as in rebuild_triangle_hit
                const float4 c0 = gld(cp, 0), c1 = gld(cp, 1), c2 = gld(cp, 2), c3 = gld(cp, 3);
                const float t0[2] = { c0.x, c0.y }, te1[2] = { c0.z, c0.w }, te2[2] = { c1.x, c1.y };
                rtxnp::triangle_outputs(I.world, rtxnp::mk(c1.z, c1.w, c2.x), rtxnp::mk(c2.y, c2.z, c2.w), rtxnp::mk(c3.x, c3.y, c3.z), t0, te1, te2, u, v, normal, tu, tv);
                material = B.material_offset + as_i(c3.w);
            }
        } else if (object < sc.instance_count + sc.sphere_count) {
            const rtx_sphere & s = sc.spheres[object - sc.instance_count];
            rtxhp::sphere_outputs(o, d, t, rtxnp::ptr3(s.center), s.radius_inv, point, normal, tu, tv);
            material = s.material_id;
        } else {
            const rtx_plane & pl = sc.planes[object - sc.instance_count - sc.sphere_count];
            rtxhp::plane_outputs(o, d, t, rtxnp::ptr3(pl.normal), rtxnp::ptr3(pl.u_axis), rtxnp::ptr3(pl.v_axis), point, normal, tu, tv);
            material = pl.material_id;
        }
    }
    query_store_channels(out, e, t, point, normal, tu, tv, material, object, triangle);
}
// entry e of a row that holds fewer hits: the values of a miss
RTX_D void hit_write_miss(const DevQuery & out, const size_t e) {
    const rtxnp::P3 zero = rtxnp::mk(0.0f, 0.0f, 0.0f);
    query_store_channels(out, e, INFINITY, zero, zero, 0.0f, 0.0f, -1, -1, -1);
}

// rows7: the m segments of the round; out: the channel arrays advanced to the round's first row (K entries per row); count: likewise, or null
template <bool LIST, bool FILTERED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_hits(const DevScene sc, const float * __restrict__ rows7, const int m, const int K, const DevQuery out, int32_t * __restrict__ count,
                  const uint64_t * __restrict__ order, int32_t * const spill_base, const int spill_threads, uint32_t * const head, const QueryMasks<FILTERED> masks) {
    __shared__ float lds_rows[7 * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ float lds_key[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ float lds_list[LIST ? 3 * rtxhp::MAX_HITS * RTX_QUERY_BLOCK : 1];
    __shared__ int lds_tile;
    NearestStack st = nearest_stack(lds_stack, lds_key, spill_base, spill_threads);
    const bool cold = out.normal || out.uv || out.material_id;                    // kernel arguments: the same for every lane
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    for (;;) {
        const int tile = query_next_tile(head, lds_tile);
        if (tile >= tiles) break;
        float r[7];
        query_slot_row<7>(order, lds_rows, rows7, m, tile, r);
        size_t p;
        if (!query_caller_row(order, m, tile * RTX_QUERY_BLOCK + threadIdx.x, p)) continue;
        rtxhp::Tally w;
        typename std::conditional<LIST, HitsList, HitsNoList>::type L;
        if constexpr (LIST) L.base = &lds_list[threadIdx.x];
        auto S = query_scene<HitsScene>(sc, masks, p);
        rtxhp::walk(S, st, L, r, LIST ? K : 0, count != nullptr, w);
        if (count) count[p] = w.count;
        if constexpr (LIST) {
            const rtxnp::P3 o = rtxnp::mk(r[0], r[1], r[2]), d = rtxnp::mk(r[3], r[4], r[5]);
            for (int j = 0; j < K; j++) {
                const size_t e = p * (size_t)K + (size_t)j;
                if (j < w.held) {
                    float t; int32_t object, triangle;
                    L.get(j, t, object, triangle);
                    hit_write(sc, out, cold, e, o, d, r[6], t, object, triangle);
                } else hit_write_miss(out, e);
            }
        }
    }
}
