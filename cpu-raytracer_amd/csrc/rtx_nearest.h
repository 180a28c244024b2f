// rtx_nearest.h — nearest-surface-point queries (include/rtx.h: rtx_query_nearest): k_query_nearest, one kernel per round — and the frame
// it shares with the other walk queries: k_query_hits (rtx_hits.h), k_query_sweep (rtx_sweep.h), k_query_overlap (rtx_overlap.h).
//
// THE FRAME, each step written once (here, and the row and channel steps in rtx_query.h); [the kernels that call it]:
//   query_next_tile    [all four]  One row per lane, RTX_QUERY_BLOCK lanes per workgroup.  A workgroup walks one tile of RTX_QUERY_BLOCK rows to the end,
//                      every lane its own row, then fetches the next tile from the round's counter (zeroed before the launch), so the grid
//                      never exceeds the threads the context's spill region was sized for.  No refill of single lanes (DESIGN.md 9,
//                      Nearest-point queries).  The kernel reads the rows and writes its outputs itself: no queue set, no resolve launch.
//   query_slot_row     [hits, sweep]  The row of slot i: staged through LDS (query_load_row), or with an order (RTX_QUERY_SORT) gathered from row
//                      key_row(order[i]) (query_gather_row).
//   query_caller_row   [hits, sweep, k_query_resolve]  (rtx_query.h) The caller's row of slot i, where the slot's answers are scattered and its row mask is read.
//   query_scene        [hits, sweep]  The Scene the walk runs on: Base (NearestScene or a Scene derived from it), or for a FILTERED instantiation
//                      Masked<Base>, which answers FILTER's predicates of rtx_nearest_math.h from the context's object-mask table and the row's
//                      mask.  FILTERED takes three more kernel arguments (QueryMasks<true>: the table or null, the row masks or null, the
//                      scalar); DevScene is the same.  The row's mask is loaded once, at the caller's row — so through the order of a sorted
//                      round like the row itself — and stays in one register; a tile's lanes set it anew.  An instance's mask is one dword at
//                      table[tlas_indices[slot]], read at the TLAS leaf ahead of the instance's 64-byte matrix; the masks of spheres and
//                      planes are read at an index every lane shares.  The unfiltered instantiation's predicates are constants.
//   nearest_stack      [nearest, hits, sweep]  Stack entries (node, key); the first RTX_LDS_STACK per lane in LDS, entry e of lane l at [e][l] like k_trace_fast's
//                      lds_stack / lds_key (one dword per lane and instruction: conflict free), deeper ones in regions 0 and 1 of the
//                      context's spill buffer, which closest-hit launches of the same stream use the same way.  At most rtxnp::stack_need()
//                      entries; the host refuses a scene that needs more than min(stack_size, RTX_MAX_STACK) before the launch, so there is
//                      no overflow path.  (k_query_overlap's stack has no key: OverlapStack, one region.)
//   query_store_answer [sweep]  The outputs of a single-answer walk: the cold record is read after the walk and only if normal, uv or
//                      material is requested (a branch on kernel arguments), then query_store_channels (rtx_query.h) with the object id of
//                      query_object_id [both: hits' hit_write, sweep, k_query_resolve].
// k_query_nearest and k_query_overlap keep the row, the caller row, the Scene and (nearest) the store block spelled out, with a comment at
// the place that names the functions they must match: through the functions they measured up to 2 % slower at the same registers, LDS and
// occupancy (profiles/walk_frame_ab_shared_*.json), and spelled out they compile to the code they were.  A change to such a step goes into
// the function AND into these two kernels.
// Every walk is the function the host twin runs (rtx_*_math.h) over the TLAS and the per-mesh BVHs in the per-lane node layout (two
// global_load_dwordx4 per node, both children of an inner node fetched together), hot triangles the same way.  The other three headers say
// only what differs: the row, the walk, the list, the stack form.
//
// k_query_nearest: rows (x, y, z, maximum distance), the walk rtxnp::walk, a distance-ordered descent.  LDS: 4 KiB of staged rows + 2 x 16 KiB.
// RTX_NEAREST_FETCH=0 (head == nullptr, this kernel only): tiles blockIdx.x, blockIdx.x + gridDim.x, ... instead of the counter (the A/B:
// DESIGN.md 9) — tiles near a dense part of the scene take many times longer than empty ones, and neighbours in a coherent order are alike.
//
// SIGNED (rtx_query_signed_distance): the instantiations that also write the signed distance and the feature code of rtx_side_math.h.  They
// take QuerySide<true> (the per-BLAS table array, the signed-distance pointer, the feature pointer or null), empty otherwise like
// QueryMasks.  The sign is computed after the walk has returned, next to the cold-record reads: the winner's matrix and three 16-byte hot
// loads, the region chain, then the mesh's 32-byte DevSideBlas entry and behind it an edge record, or a slot vertex and its record: up to
// three dependent loads (a face needs only the entry's null test).  The frame is the same; the two instantiations without it are the code
// they were.
#pragma once
#include "rtx_query.h"
#include "rtx_shade.h"
#include "rtx_nearest_math.h"
#include "rtx_side.h"

struct NearestScene {
    const DevScene & sc;
    rtx_gptr tlas, nodes, tris;
    RTX_WALK_UNFILTERED
    RTX_D int sphere_count() const { return sc.sphere_count; }
    RTX_D int plane_count() const { return sc.plane_count; }
    RTX_D int tlas_nodes() const { return sc.tlas_node_count; }
    RTX_D void sphere(int i, rtxnp::P3 & c, float & r2) const { const rtx_sphere & s = sc.spheres[i]; c = rtxnp::ptr3(s.center); r2 = s.radius_squared; }
    RTX_D void plane(int i, rtxnp::P3 & n, float & dist) const { const rtx_plane & pl = sc.planes[i]; n = rtxnp::ptr3(pl.normal); dist = pl.distance; }
    static RTX_D void node(rtx_gptr base, int i, rtxnp::P3 & mn, rtxnp::P3 & mx, int & first, int & count) {
        const float4 a = gld(base, 2 * i), b = gld(base, 2 * i + 1);
        mn = rtxnp::mk(a.x, a.y, a.z); mx = rtxnp::mk(b.x, b.y, b.z); first = as_i(a.w); count = as_i(b.w);
    }
    RTX_D void tlas_node(int i, rtxnp::P3 & mn, rtxnp::P3 & mx, int & first, int & count) const { node(tlas, i, mn, mx, first, count); }
    RTX_D void blas_node(int i, rtxnp::P3 & mn, rtxnp::P3 & mx, int & first, int & count) const { node(nodes, i, mn, mx, first, count); }
    RTX_D int enter(int slot, rtxnp::P3 p, rtxnp::P3 & pl) {
        const int inst = sc.tlas_indices[slot];
        const rtx_instance & I = sc.instances[inst];
        pl = rtxnp::xform_pos(I.world_inv, p);
        const DevBlas & B = sc.blas[I.blas_id];
        nodes = RTX_GPTR(B.nodes); tris = RTX_GPTR(B.tri_hot);
        return inst;
    }
    RTX_D void triangle(int i, rtxnp::P3 & p0, rtxnp::P3 & e1, rtxnp::P3 & e2) const {
        const float4 a = gld(tris, RTX_TRI_STRIDE * i), b = gld(tris, RTX_TRI_STRIDE * i + 1), c = gld(tris, RTX_TRI_STRIDE * i + 2);
        p0 = rtxnp::mk(a.x, a.y, a.z); e1 = rtxnp::mk(b.x, b.y, b.z); e2 = rtxnp::mk(c.x, c.y, c.z);
    }
};

// the extra kernel arguments of a FILTERED instantiation; none otherwise
template <bool FILTERED> struct QueryMasks { static constexpr bool filtered = false; };
template <> struct QueryMasks<true> { static constexpr bool filtered = true; const uint32_t * table; const uint32_t * rows; uint32_t row; };
// the mask of caller row p of the round
RTX_D uint32_t query_row_mask(const QueryMasks<true> & k, const size_t p) { return k.rows ? k.rows[p] : k.row; }

// the workgroup's next tile of the round: head is the round's counter.  Every thread of the workgroup must call this
RTX_D int query_next_tile(uint32_t * const head, int & lds_tile) {
    __syncthreads();                                                          // every lane has taken its row and the number of the previous tile
    if (threadIdx.x == 0) lds_tile = (int)atomicAdd(head, 1u);
    __syncthreads();
    return lds_tile;
}
// the row of slot i = tile * RTX_QUERY_BLOCK + threadIdx.x (zeros at and beyond m).  Every thread of the workgroup must call this
template <int ROW>
RTX_D void query_slot_row(const uint64_t * order, float (&lds)[ROW * RTX_QUERY_BLOCK], const float * rows, const int m, const int tile, float (&row)[ROW]) {
    if (order) query_gather_row<ROW>(order, rows, m, tile * RTX_QUERY_BLOCK + threadIdx.x, row);      // a kernel argument: the same branch for every lane
    else query_load_row<ROW>(lds, rows, m, row, tile);
}

// a Scene (NearestScene, HitsScene) that answers FILTER's predicates: table = the M object masks (null: all ones), row_mask = this lane's
template <typename Base> struct Masked : Base {
    const uint32_t * table; uint32_t row_mask;
    RTX_D bool row_visible() const { return row_mask != 0u; }
    RTX_D bool sphere_visible(int i) const { return !table || rtxnp::mask_visible(table[this->sc.instance_count + i], row_mask); }
    RTX_D bool plane_visible(int i) const { return !table || rtxnp::mask_visible(table[this->sc.instance_count + this->sc.sphere_count + i], row_mask); }
    RTX_D bool instance_visible(int slot) const { return !table || rtxnp::mask_visible(table[this->sc.tlas_indices[slot]], row_mask); }
};
// The Scene of the row whose caller row is p: a Base at the TLAS root, Masked with the row's mask in a FILTERED instantiation
template <typename Base> RTX_D Base query_scene(const DevScene & sc) { return Base{ NearestScene{ sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr } }; }
template <typename Base, bool FILTERED>
RTX_D auto query_scene(const DevScene & sc, const QueryMasks<FILTERED> & masks, const size_t p) {
    if constexpr (FILTERED) return Masked<Base>{ query_scene<Base>(sc), masks.table, query_row_mask(masks, p) };
    else return query_scene<Base>(sc);
}
struct NearestStack {
    int * stk; float * key; int * spill; float * spill_key; int stride;
    RTX_D void push(int sp, int node, float d2) {
        if (sp < RTX_LDS_STACK) { stk[sp * RTX_WAVE] = node; key[sp * RTX_WAVE] = d2; }
        else { spill[(sp - RTX_LDS_STACK) * stride] = node; spill_key[(sp - RTX_LDS_STACK) * stride] = d2; }
    }
    RTX_D void pop(int sp, int & node, float & d2) const {
        if (sp < RTX_LDS_STACK) { node = stk[sp * RTX_WAVE]; d2 = key[sp * RTX_WAVE]; }
        else { node = spill[(sp - RTX_LDS_STACK) * stride]; d2 = spill_key[(sp - RTX_LDS_STACK) * stride]; }
    }
};
// this lane's stack: its column of the workgroup's two LDS arrays, then its entries of regions 0 and 1 of the spill buffer
RTX_D NearestStack nearest_stack(int (&lds_stack)[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE], float (&lds_key)[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE],
                                 int32_t * const spill_base, const int spill_threads) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = blockIdx.x * RTX_QUERY_BLOCK + threadIdx.x;                  // < spill_threads: the host sizes the grid
    const size_t spill_region = (size_t)spill_threads * (RTX_MAX_STACK - RTX_LDS_STACK);
    return { &lds_stack[wave][0][lane], &lds_key[wave][0][lane], spill_base + gtid, (float *)(spill_base + spill_region) + gtid, spill_threads };
}

// the extra kernel arguments of a SIGNED instantiation (rtx_query_signed_distance); none otherwise.  blas: one DevSideBlas per BLAS id, beside
// the DevBlas table, so DevBlas / DevScene and every kernel that takes them are what they were; signed_out: n floats; feature: n or null
template <bool SIGNED> struct QuerySide { static constexpr bool is_signed = false; };
template <> struct QuerySide<true> { static constexpr bool is_signed = true; const DevSideBlas * blas; float * signed_out; int32_t * feature; };

// the tables of one mesh as SIDE of rtx_side_math.h reads them: one 16-byte load per edge, an index and a 16-byte load per vertex
struct SideTables {
    const DevSideBlas & t;
    RTX_D bool has_tables() const { return t.vert_pn != nullptr; }
    RTX_D rtxnp::P3 edge(int i) const { const float4 n = gld(RTX_GPTR(t.edge_pn), i); return rtxnp::mk(n.x, n.y, n.z); }
    RTX_D rtxnp::P3 vertex(int slot, int k) const {
        const int32_t v = t.slot_vertices[3 * (size_t)slot + k];
        if (v < 0 || v >= t.vertex_count) return rtxnp::mk(0.0f, 0.0f, 0.0f);
        const float4 n = gld(RTX_GPTR(t.vert_pn), v); return rtxnp::mk(n.x, n.y, n.z);
    }
};

// SIDE of rtx_side_math.h for the walk's answer a of the row at p: the sign and the FEATURE code.  After the walk, next to the cold-record
// reads: the instance's matrix, three 16-byte hot loads, the region chain, the mesh's table entry and at most two more dependent loads
RTX_D int nearest_side(const DevScene & sc, const DevSideBlas * side, const rtxnp::Answer & a, const rtxnp::P3 p, bool & negative) {
    negative = false;
    if (a.kind == rtxnp::KIND_TRI) {
        const rtx_instance & I = sc.instances[a.object];
        const rtx_gptr hp = RTX_GPTR(sc.blas[I.blas_id].tri_hot);
        const float4 p0 = gld(hp, RTX_TRI_STRIDE * a.slot), e1 = gld(hp, RTX_TRI_STRIDE * a.slot + 1), e2 = gld(hp, RTX_TRI_STRIDE * a.slot + 2);
        const rtxnp::P3 pl = rtxnp::xform_pos(I.world_inv, p);
        const SideTables tb = { side[I.blas_id] };
        return rtxsd::triangle_side(rtxnp::sub(pl, rtxnp::mk(p0.x, p0.y, p0.z)), rtxnp::mk(e1.x, e1.y, e1.z), rtxnp::mk(e2.x, e2.y, e2.z), a.slot, tb, negative);
    }
    if (a.kind == rtxnp::KIND_SPHERE) { const rtx_sphere & s = sc.spheres[a.object]; negative = rtxsd::sphere_side(p, rtxnp::ptr3(s.center), s.radius_squared); return rtxsd::FEATURE_SPHERE; }
    if (a.kind == rtxnp::KIND_PLANE) { const rtx_plane & pl = sc.planes[a.object]; negative = rtxsd::plane_side(p, rtxnp::ptr3(pl.normal), pl.distance); return rtxsd::FEATURE_PLANE; }
    return rtxsd::FEATURE_NONE;
}

// The channels of the one answer a (rtxnp::Answer, rtxsp::Answer) of caller row p.  query_point() is the point the sphere and plane outputs are
// taken at, distance() the distance channel of a hit; both are evaluated only where they are stored.  cold: normal, uv or material is requested
template <typename Answer, typename Point, typename Distance>
RTX_D void query_store_answer(const DevScene & sc, const DevQuery & out, const bool cold, const size_t p, const Answer & a, Point && query_point, Distance && distance) {
    const bool hit = a.kind != rtxnp::KIND_NONE;
    rtxnp::P3 point = rtxnp::mk(0.0f, 0.0f, 0.0f), normal = point;
    float tu = 0.0f, tv = 0.0f;
    int material = -1;
    if (hit && (out.position || cold)) {
        if (a.kind == rtxnp::KIND_TRI) nearest_triangle_outputs(sc, a.object, a.slot, a.u, a.v, out.position != nullptr, cold, point, normal, tu, tv, material);
        else if (a.kind == rtxnp::KIND_SPHERE) nearest_sphere_outputs(sc.spheres[a.object], query_point(), point, normal, tu, tv, material);
        else nearest_plane_outputs(sc.planes[a.object], query_point(), point, normal, tu, tv, material);
    }
    query_store_channels(out, p, out.distance && hit ? distance() : INFINITY, point, normal, tu, tv, hit ? material : -1,
                         hit ? query_object_id(sc, a.kind == rtxnp::KIND_TRI, a.kind == rtxnp::KIND_SPHERE, a.object) : -1, a.kind == rtxnp::KIND_TRI ? a.slot : -1);
}

template <bool FILTERED, bool SIGNED>
__global__ __launch_bounds__(RTX_QUERY_BLOCK)
void k_query_nearest(const DevScene sc, const float * __restrict__ rows4, const int m, const DevQuery out, const uint64_t * __restrict__ order,
                     int32_t * const spill_base, const int spill_threads, uint32_t * const head, const QueryMasks<FILTERED> masks, const QuerySide<SIGNED> side) {
    __shared__ float lds_rows[4 * RTX_QUERY_BLOCK];
    __shared__ int lds_stack[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ float lds_key[RTX_QUERY_BLOCK / RTX_WAVE][RTX_LDS_STACK][RTX_WAVE];
    __shared__ int lds_tile;
    NearestStack st = nearest_stack(lds_stack, lds_key, spill_base, spill_threads);
    const bool cold = out.normal || out.uv || out.material_id;                    // kernel arguments: the same for every lane
    const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK;
    int tile = blockIdx.x;
    for (int k = 0; ; k++) {
        if (head) tile = query_next_tile(head, lds_tile);
        else if (k) tile += gridDim.x;                                            // RTX_NEAREST_FETCH=0: tiles by stride, no counter
        if (tile >= tiles) break;
        const int i = tile * RTX_QUERY_BLOCK + threadIdx.x;
        float r[4];
        // From here to the stores: query_slot_row<4>, query_caller_row, query_scene and query_store_answer (q = the query point, distance =
        // root(d2)) spelled out; they must match those functions (the header comment says why).  The stride path has a barrier of its own
        if (order) query_gather_row<4>(order, rows4, m, i, r);
        else {
            if (!head && k) __syncthreads();                                      // tiles by stride: every lane has taken its row of the previous tile
            query_load_row<4>(lds_rows, rows4, m, r, tile);
        }
        if (i >= m) continue;
        rtxnp::Answer a;
        if constexpr (FILTERED) {
            const size_t pr = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;
            Masked<NearestScene> S = { { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr }, masks.table, pr < (size_t)m ? query_row_mask(masks, pr) : 0u };
            rtxnp::walk(S, st, r, a);
        } else {
            NearestScene S = { sc, RTX_GPTR(sc.tlas_nodes), nullptr, nullptr };
            rtxnp::walk(S, st, r, a);
        }
        const size_t p = order ? (size_t)rtxq::key_row(order[i]) : (size_t)i;      // the caller's row of this slot
        if (p >= (size_t)m) continue;                                              // never: a sorted key holds a row of the round
        const bool hit = a.kind != rtxnp::KIND_NONE;
        rtxnp::P3 point = rtxnp::mk(0.0f, 0.0f, 0.0f), normal = point;
        float tu = 0.0f, tv = 0.0f;
        int material = -1;
        if (hit && (out.position || cold)) {
            const rtxnp::P3 q = rtxnp::mk(r[0], r[1], r[2]);
            if (a.kind == rtxnp::KIND_TRI) nearest_triangle_outputs(sc, a.object, a.slot, a.u, a.v, out.position != nullptr, cold, point, normal, tu, tv, material);
            else if (a.kind == rtxnp::KIND_SPHERE) nearest_sphere_outputs(sc.spheres[a.object], q, point, normal, tu, tv, material);
            else nearest_plane_outputs(sc.planes[a.object], q, point, normal, tu, tv, material);
        }
        if (out.distance) out.distance[p] = hit ? rtxnp::root(a.d2) : INFINITY;
        if (out.position) { out.position[3 * p + 0] = point.x; out.position[3 * p + 1] = point.y; out.position[3 * p + 2] = point.z; }
        if (out.normal) { out.normal[3 * p + 0] = normal.x; out.normal[3 * p + 1] = normal.y; out.normal[3 * p + 2] = normal.z; }
        if (out.uv) { out.uv[2 * p + 0] = tu; out.uv[2 * p + 1] = tv; }
        if (out.material_id) out.material_id[p] = hit ? material : -1;
        if (out.object_id)
            out.object_id[p] = !hit ? -1 : a.kind == rtxnp::KIND_TRI ? a.object : a.kind == rtxnp::KIND_SPHERE ? sc.instance_count + a.object : sc.instance_count + sc.sphere_count + a.object;
        if (out.triangle_id) out.triangle_id[p] = a.kind == rtxnp::KIND_TRI ? a.slot : -1;
        if constexpr (SIGNED) {
            bool negative;
            const int feature = nearest_side(sc, side.blas, a, rtxnp::mk(r[0], r[1], r[2]), negative);
            side.signed_out[p] = hit ? rtxsd::signed_distance(a.d2, negative) : INFINITY;
            if (side.feature) side.feature[p] = feature;
        }
    }
}
