// rtx_query.h — ray queries (include/rtx.h: rtx_query_closest / rtx_query_occluded): the kernels around the traversal kernels.
//
//   k_query_fill            n x 6 floats (origin, direction)               -> ray records of level 1 of the query's own queue set
//   k_query_resolve         hit records of that level                      -> the requested channels, one array each
//   k_query_fill_segments   n x 7 floats (origin, direction, max distance) -> ONE explicit shadow segment of level 0 (q.shadow_explicit)
//   k_query_store_occluded  that segment's occlusion flags                 -> int32 1 / 0
//
//   k_query_sort_bounds     RTX_QUERY_SORT: the rows of a round -> the twelve bounds of their six key coordinates (rtx_query_sort_math.h)
//   k_query_sort_keys       the rows and those bounds -> one 64-bit key per row; rocPRIM's radix sort of the keys runs between this and the fill
//
// The walk in between is the production kernel of the render path, launched as a frame launches it (rtx_api.hip): a closest-hit launch over
// level 1, a shadow-ray launch over level 0.  All four kernels stream: one slot per lane, a chunk (<= RTX_QUERY_CHUNK_RAYS rows) per launch.
// The unit-test hooks rtx_debug_trace_rays / rtx_debug_occluded run the same rounds, so the rules below are theirs too.
//
// No ray: a row whose direction is (+-0, +-0, +-0), as for ray views (primary_pixel_v, rtx_trace.h).  Its slot is marked RAY_DEAD_PIXEL (not
// NF_LIT for a segment), which both closest-hit kernels answer with the record of a clipped pixel: a miss.
// Not walked either: a row with a NaN or infinite origin or direction component.  It hits nothing in the reference's arithmetic — every hit
// test ends in a comparison with a NaN, a zero or an infinite distance (ray_is_finite, rtx_trace.h) — so a miss is its answer, and the
// packet kernels must not be given it: their NaN-free slab test is chosen by the inverse direction alone and would pass every box of a NaN
// origin, padding slots included.  Level 0 of a ray view filters the same rays (k_packet); here the fill does.  A segment whose maximum
// distance is NaN is never occluded (t < NaN is false for every t) and is not walked; a negative one is skipped by the shadow-ray kernels
// themselves and keeps the 0 the fill stored.
#pragma once
#include "rtx_device.h"
#include "rtx_query_sort_math.h"

#define RTX_QUERY_BLOCK 256

// the channel targets of one chunk (the caller's arrays, advanced to the chunk's first ray): null = not requested
struct DevQuery {
    float * distance; float * position; float * normal; float * uv;
    int32_t * material_id; int32_t * object_id; int32_t * triangle_id;
};
// element e of every requested channel (V: v3 or rtxnp::P3); every kernel that answers into a DevQuery stores through here
template <typename V>
RTX_D void query_store_channels(const DevQuery & out, const size_t e, const float distance, const V & point, const V & normal, const float tu, const float tv,
                                const int material, const int object, const int triangle) {
    if (out.distance) out.distance[e] = distance;
    if (out.position) { out.position[3 * e + 0] = point.x; out.position[3 * e + 1] = point.y; out.position[3 * e + 2] = point.z; }
    if (out.normal) { out.normal[3 * e + 0] = normal.x; out.normal[3 * e + 1] = normal.y; out.normal[3 * e + 2] = normal.z; }
    if (out.uv) { out.uv[2 * e + 0] = tu; out.uv[2 * e + 1] = tv; }
    if (out.material_id) out.material_id[e] = material;
    if (out.object_id) out.object_id[e] = object;
    if (out.triangle_id) out.triangle_id[e] = triangle;
}
// the object_id channel of instance / sphere / plane `index`: instances, then spheres, then planes, the numbering of RTX_AOV_OBJECT_ID (k_shade).
// At most one of triangle, sphere is set; neither: a plane
RTX_D int query_object_id(const DevScene & sc, const bool triangle, const bool sphere, const int index) {
    return triangle ? index : sphere ? sc.instance_count + index : sc.instance_count + sc.sphere_count + index;
}

// Rows of ROW floats are 24 / 28 bytes: lane-per-row loads would be ROW loads of stride ROW * 4 B per lane.  The workgroup reads its
// RTX_QUERY_BLOCK rows as one contiguous run of floats instead (consecutive lanes, consecutive dwords; any 4-byte aligned address) into LDS,
// and every lane takes its row from there.  Rows at and beyond m read as zeros: no ray.  Every thread of the workgroup must call this.
// `block`: the tile of RTX_QUERY_BLOCK rows to stage — the workgroup's own, or the one a workgroup that loops over tiles is at (k_query_nearest).
template <int ROW>
RTX_D void query_load_row(float (&lds)[ROW * RTX_QUERY_BLOCK], const float * __restrict__ rows, const int m, float (&row)[ROW], const int block = blockIdx.x) {
    const int first = block * RTX_QUERY_BLOCK;
    const int have = (m - first < RTX_QUERY_BLOCK ? (m - first > 0 ? m - first : 0) : RTX_QUERY_BLOCK) * ROW;      // floats of this workgroup's rows
    const float * const src = rows + (size_t)first * ROW;
    for (int k = threadIdx.x; k < ROW * RTX_QUERY_BLOCK; k += RTX_QUERY_BLOCK) lds[k] = k < have ? src[k] : 0.0f;
    __syncthreads();
    for (int k = 0; k < ROW; k++) row[k] = lds[threadIdx.x * ROW + k];
}
RTX_D bool query_row_is_ray(const v3 o, const v3 d) {
    return !((d.x == 0.0f) & (d.y == 0.0f) & (d.z == 0.0f)) && ray_is_finite(o, d);
}

// RTX_QUERY_SORT.  `order` is the round's sorted keys (rtxq::sort_key): slot i traces caller row rtxq::key_row(order[i]), and the answer of
// slot i goes back to that row.  A null order is the caller's order, slot i = row i, through the staging above.
// The row of slot i with an order: ROW dword loads at the row's own address (any 4-byte aligned address: no wider load is legal).  Slots at
// and beyond m read as zeros, as in query_load_row.
template <int ROW>
RTX_D void query_gather_row(const uint64_t * __restrict__ order, const float * __restrict__ rows, const int m, const int i, float (&row)[ROW]) {
    const uint32_t at = i < m ? rtxq::key_row(order[i]) : (uint32_t)m;      // < m for every key the key kernel wrote: nothing else is ever read
    if (at < (uint32_t)m) {
        const float * const src = rows + (size_t)at * ROW;
        for (int k = 0; k < ROW; k++) row[k] = src[k];
    } else for (int k = 0; k < ROW; k++) row[k] = 0.0f;
}
// The caller's row p of slot i of a round of m rows: where the slot's answer goes, and where a filtered walk query reads its row mask.
// false: the slot carries no row — i >= m, or (never: a sorted key holds a row of the round) a key whose row is none of the round's
RTX_D bool query_caller_row(const uint64_t * order, const int m, const int i, size_t & p) {
    if (i >= m) return false;
    p = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;
    return p < (size_t)m;
}

// The twelve bounds of a round's live rows, bounds[0..5] the minima as ordered keys, bounds[6..11] the maxima as complemented ordered keys:
// both reduce by an unsigned min, one memset of 0xff per round initialises them (upd_reduce_bounds, rtx_update.h, does the same for six).
// wave64 min, then at most one atomic per wave and bound: a wave that cannot lower the bound it reads does not issue one.  Measured
// (DESIGN.md 9): 170 - 270 us per 2^20 rows all the same — as a sweep over an image proceeds most waves still improve a bound, and twelve
// words of one cache line sustain few atomics and loads per microsecond.  A reduction per workgroup over several tiles is the next step.
template <int ROW>
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_sort_bounds(const float * __restrict__ rows, const int m, uint32_t * __restrict__ bounds) {
    __shared__ float lds[ROW * RTX_QUERY_BLOCK];
    float r[ROW];
    query_load_row<ROW>(lds, rows, m, r);
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    uint32_t k12[2 * rtxq::COORDS];
    for (int a = 0; a < 2 * rtxq::COORDS; a++) k12[a] = 0xffffffffu;
    if (i < m && rtxq::row_is_live(r, ROW)) { float x[rtxq::COORDS]; rtxq::coordinates(r, ROW, x); rtxq::bounds_of_row(x, k12); }
    for (int a = 0; a < 2 * rtxq::COORDS; a++) {
        uint32_t v = k12[a];
        for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64); v = w < v ? w : v; }
        if ((threadIdx.x & 63) == 0 && v < __hip_atomic_load(&bounds[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&bounds[a], v);
    }
}

// keys[i] = rtxq::sort_key of row i.  The bounds are the same twelve words for every lane: scalar loads, one plan per wave.
template <int ROW>
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_sort_keys(const float * __restrict__ rows, const int m, const uint32_t * __restrict__ bounds, uint64_t * __restrict__ keys) {
    __shared__ float lds[ROW * RTX_QUERY_BLOCK];
    float r[ROW];
    query_load_row<ROW>(lds, rows, m, r);
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (i >= m) return;
    const rtxq::Plan plan = rtxq::make_plan(bounds);
    keys[i] = rtxq::sort_key(plan, r, ROW, (uint32_t)i);
}

// The same two kernels for rows whose key is taken over their first KEY floats only (rtx_query_sweep: the 7-float key of 8-float rows): the
// row stride stays ROW.  Copies, not wrappers over one body with the two above: written that way (the body a forced-inline function, the LDS
// array passed in or declared in it) hipcc allocates k_query_sort_bounds<4> 18 VGPRs instead of 22, and the ray queries' kernels are to
// stay the code they were measured as.  A change to the reduction or the atomic guard goes into both pairs.
template <int ROW, int KEY>
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_sort_bounds_of(const float * __restrict__ rows, const int m, uint32_t * __restrict__ bounds) {
    __shared__ float lds[ROW * RTX_QUERY_BLOCK];
    float r[ROW];
    query_load_row<ROW>(lds, rows, m, r);
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    uint32_t k12[2 * rtxq::COORDS];
    for (int a = 0; a < 2 * rtxq::COORDS; a++) k12[a] = 0xffffffffu;
    if (i < m && rtxq::row_is_live(r, KEY)) { float x[rtxq::COORDS]; rtxq::coordinates(r, KEY, x); rtxq::bounds_of_row(x, k12); }
    for (int a = 0; a < 2 * rtxq::COORDS; a++) {
        uint32_t v = k12[a];
        for (int o = 32; o > 0; o >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64); v = w < v ? w : v; }
        if ((threadIdx.x & 63) == 0 && v < __hip_atomic_load(&bounds[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&bounds[a], v);
    }
}
template <int ROW, int KEY>
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_sort_keys_of(const float * __restrict__ rows, const int m, const uint32_t * __restrict__ bounds, uint64_t * __restrict__ keys) {
    __shared__ float lds[ROW * RTX_QUERY_BLOCK];
    float r[ROW];
    query_load_row<ROW>(lds, rows, m, r);
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (i >= m) return;
    const rtxq::Plan plan = rtxq::make_plan(bounds);
    keys[i] = rtxq::sort_key(plan, r, KEY, (uint32_t)i);
}

// the caller row of every slot of a sorted round, for rtx_debug_query_order: order_out[i] = first + row
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_sort_order(const uint64_t * __restrict__ order, const int m, const int32_t first, int32_t * __restrict__ order_out) {
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (i < m) order_out[i] = first + (int32_t)rtxq::key_row(order[i]);
}

// slots [0, m rounded up to a packet) of level 1: the chunk's rays with zero differentials (r2 .. r4 are neither written nor read: the
// traversal kernels take origin and direction, k_query_resolve knows the differentials are zero), pixel = the slot, parent -1
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_fill(const DevQueues q, const float * __restrict__ rays6, const int m, const uint64_t * __restrict__ order) {
    __shared__ float lds[6 * RTX_QUERY_BLOCK];
    float r[6];
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (order) query_gather_row<6>(order, rays6, m, i, r);      // a kernel argument: the same branch for every lane
    else query_load_row<6>(lds, rays6, m, r);
    if (i == 0) q.counters->ray_count[1] = (uint32_t)m;
    if (i >= ((m + RTX_WAVE - 1) & ~(RTX_WAVE - 1))) return;
    const bool live = i < m && query_row_is_ray(V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5]));
    const uint32_t s = (uint32_t)q.level_base[1] + (uint32_t)i;
    q.r0[s] = make_float4(r[0], r[1], r[2], r[3]);
    q.r1[s] = make_float4(r[4], r[5], as_f(live ? i : RAY_DEAD_PIXEL), as_f(-1));
}

// Distance and ids come out of the hit record: t, the primitive word, the triangle index, and for the material one word of the
// primitive.  Position, normal and uv are RayHit fields the accept branches compute: the rebuild functions of the shading pass
// (rtx_shade.h), entered only when one of the three is requested — a branch on kernel arguments, the same for every lane.
// sc.diff_enabled is 0 here (the caller clears it in its copy): the rebuild's differential block feeds none of the channels.
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_resolve(const DevScene sc, const DevQueues q, const int m, const DevQuery out, const uint64_t * __restrict__ order) {
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = (uint32_t)q.level_base[1] + (uint32_t)i;
    const float4 h0 = q.h0[s];
    const int tri = q.h1[s], prim = as_i(h0.w), kind = PRIM_KIND(prim), pi = PRIM_INDEX(prim);
    const bool is_hit = kind != PRIM_NONE;
    HitFull h; h.material_id = 0;
    h.point = h.normal = h.dO_dx = h.dO_dy = h.dN_dx = h.dN_dy = V3(0, 0, 0); h.u = h.v = h.ds_dx = h.ds_dy = h.dt_dx = h.dt_dy = 0.0f;
    const bool rebuild = out.position || out.normal || out.uv;
    if (rebuild) {
        if (is_hit) {
            const float4 r0 = q.r0[s], r1 = q.r1[s];
            RayFull ray;
            ray.o = V3(r0.x, r0.y, r0.z); ray.d = V3(r0.w, r1.x, r1.y);
            ray.dO_dx = ray.dO_dy = ray.dD_dx = ray.dD_dy = V3(0, 0, 0);
            if (kind == PRIM_TRI) rebuild_triangle_hit(sc, pi, tri, h0.x, h0.y, h0.z, ray, h);
            else if (kind == PRIM_SPHERE) rebuild_sphere_hit(sc, sc.spheres[pi], h0.x, ray, h);
            else rebuild_plane_hit(sc, sc.planes[pi], h0.x, ray, h);
        }
    } else if (out.material_id && is_hit) {
        if (kind == PRIM_TRI) {
            const DevBlas & B = sc.blas[sc.instances[pi].blas_id];
            h.material_id = B.material_offset + B.tri_cold[tri].material_id;
        } else h.material_id = kind == PRIM_SPHERE ? sc.spheres[pi].material_id : sc.planes[pi].material_id;
    }
    size_t p;
    if (!query_caller_row(order, m, i, p)) return;
    query_store_channels(out, p, is_hit ? h0.x : INFINITY, h.point, h.normal, h.u, h.v, is_hit ? h.material_id : -1,
                         is_hit ? query_object_id(sc, kind == PRIM_TRI, kind == PRIM_SPHERE, pi) : -1, (is_hit && kind == PRIM_TRI) ? tri : -1);
}

// slots [0, m rounded up to a packet) of level 0 and of its one shadow segment (the caller's DevScene copy says light_count = 1, whatever
// the frame holds): the node record only says whether the slot carries a segment (NF_LIT, shadow_slot_is_lit), the flag starts at 0
__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_fill_segments(const DevQueues q, const float * __restrict__ segments7, const int m, const uint64_t * __restrict__ order) {
    __shared__ float lds[7 * RTX_QUERY_BLOCK];
    float r[7];
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (order) query_gather_row<7>(order, segments7, m, i, r);
    else query_load_row<7>(lds, segments7, m, r);
    if (i == 0) q.counters->ray_count[0] = (uint32_t)m;
    if (i >= ((m + RTX_WAVE - 1) & ~(RTX_WAVE - 1))) return;
    const bool live = i < m && query_row_is_ray(V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5])) && r[6] == r[6];
    const uint32_t s = (uint32_t)q.shadow_base[0] + (uint32_t)i;
    q.n0[(uint32_t)q.level_base[0] + (uint32_t)i] = make_float4(0.0f, 0.0f, 0.0f, as_f(live ? (NF_HIT | NF_LIT) : 0));
    q.s0[s] = make_float4(r[0], r[1], r[2], r[6]);
    q.s1[s] = make_float4(r[3], r[4], r[5], 0.0f);
    q.socc[s] = 0u;
}

__global__ __launch_bounds__(RTX_QUERY_BLOCK) void k_query_store_occluded(const DevQueues q, const int m, int32_t * __restrict__ occluded, const uint64_t * __restrict__ order) {
    const int i = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint32_t p = order ? rtxq::key_row(order[i]) : (uint32_t)i;
    if (p < (uint32_t)m) occluded[p] = q.socc[(uint32_t)q.shadow_base[0] + (uint32_t)i] != 0u ? 1 : 0;
}
