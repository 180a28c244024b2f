// rtx_layout.h — the device node layouts, each written once: what the host conversion at upload (rtx_layout_host.h) and the refit, build and
// update kernels (rtx_refit.h, rtx_build.h, rtx_update.h) store, and what the traversal kernels read with hand-written assembly
// (rtx_packet.h).  Written once and compiled twice like rtx_update_math.h: by hipcc into the kernels and the library's host side, and by the
// host compiler into csrc/layout_check.cpp, which pins every record here bit for bit.  No HIP header; no address comes from float data.
//
//   lane record    2 quads per node: (min.x, min.y, min.z, left_or_first) (max.x, max.y, max.z, count)            [per-lane kernels, rtx_trace.h]
//   packet record  2 quads per node: (min.x, min.y, max.x, max.y) (min.z, max.z, left_or_first, count) — every SGPR pair of a fetched node is
//                  one operand of a packed-fp32 instruction                                                       [packet kernels, rtx_packet.h]
//   4-wide slot    the packet record's row with other words: (min.x, min.y, max.x, max.y) (min.z, max.z, first, meta); four slots per record,
//                  the record of inner node j at row 2 * (left child of j).  pk4 (shadow rays): meta = leaf count.  pk4c (closest hit): pk4c_meta
//   packed entries one word per pending node on the per-lane walks' stacks and work lists: ref_* (binary walks), wide_* (pk4 walks)  [both]
//   plane keys     per axis 2 floats per node, (min, max), NaN -> +inf: the unsorted input of the plane lists plane_member searches
#pragma once
#include <stddef.h>
#include "../../include/rtx.h"
#include "rtx_update_math.h"

#define RTX_REFIT_UNREACHABLE (-2)         // parent[] of a node slot no traversal reaches: its bytes stay

namespace rtxl {

using rtxu::Box;

#if defined(__HIPCC__)
using Quad = float4;                        // every record store is one 16-byte vector store
#else
struct alignas(16) Quad { float x, y, z, w; };
#endif

RTX_HD float word(int32_t v) { float f; __builtin_memcpy(&f, &v, 4); return f; }
RTX_HD int32_t word_of(float f) { int32_t v; __builtin_memcpy(&v, &f, 4); return v; }

// ---- lane record ---------------------------------------------------------------------------------------------------------------------------
RTX_HD void store_lane(Quad * nodes, size_t i, const Box & b, float left_or_first, float count) {
    nodes[2 * i]     = Quad{ b.mn[0], b.mn[1], b.mn[2], left_or_first };
    nodes[2 * i + 1] = Quad{ b.mx[0], b.mx[1], b.mx[2], count };
}
RTX_HD Box lane_box(const Quad & a, const Quad & c) {
    Box b; b.mn[0] = a.x; b.mn[1] = a.y; b.mn[2] = a.z; b.mx[0] = c.x; b.mx[1] = c.y; b.mx[2] = c.z;
    return b;
}
RTX_HD Box load_box(const Quad * nodes, size_t i) { return lane_box(nodes[2 * i], nodes[2 * i + 1]); }

// the reference's node record to the lane record and back
RTX_HD void lane_from_node(Quad * nodes, size_t i, const rtx_bvh_node & n) {
    Box b;
    for (int a = 0; a < 3; a++) { b.mn[a] = n.aabb_min[a]; b.mx[a] = n.aabb_max[a]; }
    store_lane(nodes, i, b, word(n.left_or_first), word(n.count));
}
RTX_HD void node_from_lane(const Quad * nodes, size_t i, rtx_bvh_node & n) {
    const Quad a = nodes[2 * i], c = nodes[2 * i + 1];
    const Box b = lane_box(a, c);
    for (int k = 0; k < 3; k++) { n.aabb_min[k] = b.mn[k]; n.aabb_max[k] = b.mx[k]; }
    n.left_or_first = word_of(a.w); n.count = word_of(c.w);
}

// ---- packet record, and one slot of a 4-wide record ----------------------------------------------------------------------------------------
RTX_HD void store_packet(Quad * rows, size_t i, const Box & b, float w6, float w7) {
    rows[2 * i]     = Quad{ b.mn[0], b.mn[1], b.mx[0], b.mx[1] };
    rows[2 * i + 1] = Quad{ b.mn[2], b.mx[2], w6, w7 };
}
RTX_HD void packet_from_node(Quad * rows, size_t i, const rtx_bvh_node & n, int32_t w6, int32_t w7) {
    Box b;
    for (int a = 0; a < 3; a++) { b.mn[a] = n.aabb_min[a]; b.mx[a] = n.aabb_max[a]; }
    store_packet(rows, i, b, word(w6), word(w7));
}
// one slot of a 4-wide record: the box of the node it carries, the first and meta words kept
RTX_HD void store_wide_box(Quad * rows, size_t s, const Box & b) {
    const Quad q = rows[2 * s + 1];
    store_packet(rows, s, b, q.z, q.w);
}
// both layouts of one node slot; a hole is the zero box with zero words
RTX_HD void store_node(Quad * nodes, Quad * pk_nodes, size_t i, const Box & b, int32_t left_or_first, int32_t count) {
    store_lane(nodes, i, b, word(left_or_first), word(count));
    store_packet(pk_nodes, i, b, word(left_or_first), word(count));
}
RTX_HD void store_hole(Quad * nodes, Quad * pk_nodes, size_t i) { store_node(nodes, pk_nodes, i, Box{ { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } }, 0, 0); }

// pk4c meta word of record slot s (0 .. 3; slots 0-1 lie under the record node's left child, 2-3 under its right one): leaf count | axis of
// the slot's parent << 26 | axis of the slot node << 30.  slot_count = the slot node's count word; child_count = the count word of the record
// node's child the slot lies under — the slot's parent, or the slot itself when that child is a leaf, which carries no parent axis.  The
// parent's axis rides in the first slot of its pair only.
RTX_HD uint32_t pk4c_meta(uint32_t slot_count, uint32_t child_count, int s) {
    const bool parent_axis = (s & 1) == 0 && (child_count & 0x3fffffffu) == 0u;
    return (slot_count & 0x3fffffffu) | (parent_axis ? (child_count >> 30) << 26 : 0u) | ((slot_count >> 30) << 30);
}

// ---- stack and work-list entries of the per-lane walks: a node that passed its ray's slab test, as one word -----------------------------------
// leaf reference (binary walks: k_trace_fast, pk_lane_phase_any, pk_lane_phase_closest; the work lists): the node's own words,
// REF_PACKED | axis << 28 | leaf count << 24 | first — nothing to fetch before its children / triangles.  count_word = leaf count | axis << 30.
// It fits when first < 2^24 and the leaf count < 16; a node that does not fit travels as its index (< 2^24, so bit 30 is clear) and is read back.
// The asm walkers of rtx_packet.h spell the same bits (PKB_DEFER of pk_blas_any_asm, PK_ASM_REF).
constexpr uint32_t REF_PACKED = 0x40000000u;
RTX_HD bool ref_fits(uint32_t first, uint32_t count_word) { return first < (1u << 24) && (count_word & 0x3fffffffu) < 16u; }
RTX_HD int32_t ref_pack(uint32_t first, uint32_t count_word) {
    return (int32_t)(REF_PACKED | ((count_word >> 30) << 28) | ((count_word & 0x3fffffffu) << 24) | first);
}
// of a pk4c slot (first, meta = pk4c_meta): its parent-axis bits are not the node's; build_nodes_pk4c admits only trees whose every node fits
RTX_HD int32_t ref_pack_meta(uint32_t first, uint32_t meta) { return ref_pack(first, meta & 0xc000000fu); }
RTX_HD bool ref_is_packed(int32_t e) { return (e & (int32_t)REF_PACKED) != 0; }
RTX_HD int32_t ref_first(int32_t e) { return e & 0x00ffffff; }
RTX_HD int32_t ref_count_word(int32_t e) { return (int32_t)((((uint32_t)e >> 28) & 3u) << 30) | ((e >> 24) & 15); }
// 4-wide entry (pk4 walks: pk_lane_phase_any4, k_items and the items pk_blas_any_asm4 writes): leaf count << 24 | first, no axis — any order
// is exact for shadow rays.  build_nodes_pk4 admits only trees whose every node fits: first < 2^24, leaf count < 256.
RTX_HD bool wide_fits(uint32_t first, uint32_t count) { return first < (1u << 24) && count < 256u; }
RTX_HD int32_t wide_pack(uint32_t first, uint32_t count) { return (int32_t)((count << 24) | first); }
RTX_HD int32_t wide_first(int32_t e) { return e & 0x00ffffff; }
RTX_HD int32_t wide_count(int32_t e) { return (int32_t)((uint32_t)e >> 24); }

// ---- plane keys ----------------------------------------------------------------------------------------------------------------------------
RTX_HD float plane_key(float v) { return v != v ? INFINITY : v; }
RTX_HD void store_plane_keys(float * keys, size_t i, float lo, float hi) {
#if defined(__HIPCC__)
    *(float2 *)(keys + 2 * i) = make_float2(plane_key(lo), plane_key(hi));
#else
    keys[2 * i] = plane_key(lo); keys[2 * i + 1] = plane_key(hi);
#endif
}

// ---- the pass a refit and a build end with, for index i of 2 * node_count + 4 -----------------------------------------------------------
// i < node_count: the packet record of node i from its lane record, and its six plane keys.  Unreachable slots keep their packet bytes, and
// their planes stay in the lists: a superset only sends a ray to the reference-form walker.  Every i: the box of the node that record slot
// i of pk4 / pk4c carries (slot maps made at upload), the first and meta words kept — or, with axis_fields, the pk4c meta word composed
// anew from the count words a build has just written: the record's node has its children at row / 2 of the record, + 1.
// View: DevRefit (rtx_refit.h) or its host-side like — nodes, pk_nodes, pk4_nodes, pk4c_nodes, parent, map4, map4c, plane_keys[3], node_count.
template <typename View> RTX_HD void finish_index(const View & r, int i, bool axis_fields) {
    if (i < r.node_count) {
        const Quad a = r.nodes[2 * (size_t)i], c = r.nodes[2 * (size_t)i + 1];
        if (r.parent[i] != RTX_REFIT_UNREACHABLE) store_packet(r.pk_nodes, i, lane_box(a, c), a.w, c.w);
        store_plane_keys(r.plane_keys[0], i, a.x, c.x);
        store_plane_keys(r.plane_keys[1], i, a.y, c.y);
        store_plane_keys(r.plane_keys[2], i, a.z, c.z);
    }
    if (i >= 2 * r.node_count + 4) return;
    if (r.map4) { const int j = r.map4[i]; if (j >= 0) store_wide_box(r.pk4_nodes, i, load_box(r.nodes, j)); }
    if (r.map4c) {
        const int j = r.map4c[i];
        if (j < 0) return;
        if (!axis_fields) { store_wide_box(r.pk4c_nodes, i, load_box(r.nodes, j)); return; }
        const int s = i & 3, child = ((i - s) >> 1) + (s >> 1);
        const uint32_t meta = pk4c_meta((uint32_t)word_of(r.nodes[2 * (size_t)j + 1].w), (uint32_t)word_of(r.nodes[2 * (size_t)child + 1].w), s);
        store_packet(r.pk4c_nodes, i, load_box(r.nodes, j), r.pk4c_nodes[2 * (size_t)i + 1].z, word((int32_t)meta));
    }
}

}  // namespace rtxl
