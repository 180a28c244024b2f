// rtx_layout_host.h — a tree in the reference's arrays (rtx_bvh_node) to the device node layouts of rtx_layout.h, on the host: what
// rtx_upload_blas, rtx_set_frame and rtx_alloc_blas (rtx_api.hip) upload, and the tables a refit plan is made of.  Nothing here touches a
// context or HIP, so csrc/layout_check.cpp runs the same code under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "rtx_layout.h"
#include "rtx_build_math.h"

using rtxl::Quad;

static void convert_nodes(const rtx_bvh_node * nodes, int n, std::vector<Quad> & out) {
    out.resize((size_t)2 * (n > 0 ? n : 1));
    for (int i = 0; i < n; i++) rtxl::lane_from_node(out.data(), i, nodes[i]);
}

// the packet kernels' node record (rtx_layout.h)
static void convert_nodes_pk(const rtx_bvh_node * nodes, int n, std::vector<Quad> & out) {
    out.resize((size_t)2 * (n > 0 ? n : 1));
    for (int i = 0; i < n; i++) rtxl::packet_from_node(out.data(), i, nodes[i], nodes[i].left_or_first, nodes[i].count);
}

// The shadow-ray packet walk's 4-wide node records (rtx_packet.h, pk_blas_any_asm4).  BottomLevelBVH::intersect (BottomLevelBVH.cpp:398-437)
// answers "is any triangle hit": the answer does not depend on the order the tree is walked in, and when every child box lies inside its
// parent's box — componentwise, in the stored floats — it does not depend on the inner nodes either: AABB::intersect (AABB.cpp:38-52) is
// monotone under nesting in floating point (x -> fl(x - o) and x -> fl(x * inv) are monotone, so t_near(parent) <= t_near(child) and
// t_far(child) <= t_far(parent) hold exactly, and a ray that passes a child's strict test passes its parent's).  The set of leaves a ray
// reaches is therefore the set of leaves whose own box it passes together with all ancestors' = (under nesting) the leaves reached through
// ANY subset of the ancestors.  The record of inner node j lists its grandchildren (children where a child is a leaf): the packet walk
// tests 4 boxes per fetch and takes half the dependent steps.  Trees that are not nested (or exceed the packed-entry limits) keep the
// binary walk.  Slot order = visiting order: largest box first (the likeliest occluder), unless that would need too many packet-stack entries
// at this node — then smallest stack need first, which bounds the occupancy by the tree's Strahler-like number.  *stack_need = the bound;
// max_need = the packet-stack entries a BLAS walk may need (RTX_PK4_MAX_NEED, rtx_packet.h).
//   record (128 B, at byte offset 64 * left-child index of j): 4 x { min.x, min.y, max.x, max.y, min.z, max.z, first, leaf count };
//   first = left-child index of the slot node (inner, count 0) or first triangle (leaf); unused slots hold a point box, which never passes.
// slot_map (may be null): for every record slot (index 2 * left + s of 2n + 4) the node whose box it carries, -1 for an unused slot (rtx_refit.h)
static bool build_nodes_pk4(const rtx_bvh_node * nodes, int n, int tri_count, std::vector<Quad> & out, int * stack_need, int order_mode, int max_need, std::vector<int32_t> * slot_map = nullptr) {
    if (n >= (1 << 24) || tri_count >= (1 << 24)) return false;
    auto inside = [&](int c, int p) {
        for (int a = 0; a < 3; a++) if (!(nodes[c].aabb_min[a] >= nodes[p].aabb_min[a] && nodes[c].aabb_max[a] <= nodes[p].aabb_max[a])) return false;
        return true;
    };
    // reachable inner nodes in pre-order (validate_tree has already checked the structure)
    std::vector<int> order, stack(1, 0);
    while (!stack.empty()) {
        const int i = stack.back(); stack.pop_back();
        const int cnt = nodes[i].count & 0x3fffffff, f = nodes[i].left_or_first;
        for (int a = 0; a < 3; a++) if (!(nodes[i].aabb_min[a] <= nodes[i].aabb_max[a])) return false;      // the sign-coherent slab test relies on min <= max
        if (cnt > 0) { if (!rtxl::wide_fits((uint32_t)f, (uint32_t)cnt)) return false; continue; }      // stack entries and items pack (first, count) into one word
        if (f & 1) return false;                                   // records are addressed by left / 2
        if (!inside(f, i) || !inside(f + 1, i)) return false;      // nesting
        order.push_back(i); stack.push_back(f); stack.push_back(f + 1);
    }
    out.assign((size_t)4 * (n > 0 ? n : 1) + 8, Quad{ 0.0f, 0.0f, 0.0f, 0.0f });
    if (slot_map) slot_map->assign((size_t)2 * (n > 0 ? n : 1) + 4, -1);
    std::vector<int> need((size_t)n, 0);                            // packet-stack entries the walk of a subtree can have pending
    // visiting order = slot order.  For a shadow ray any hit ends the walk, so the likeliest occluder should come first: largest box first
    // (merged launch 0.652 -> 0.627 ms; by triangle count, density or an RTSAH-style area^2 / cost key: 0.635-0.70).  Where that order would
    // need more packet-stack entries than the cap, the node falls back to the order that minimises the need (smallest need first).
    // order_mode (RTX_PK4_ORDER) 0: always smallest need first (A/B runs)
    auto area = [&](int i) { const double dx = (double)nodes[i].aabb_max[0] - nodes[i].aabb_min[0], dy = (double)nodes[i].aabb_max[1] - nodes[i].aabb_min[1], dz = (double)nodes[i].aabb_max[2] - nodes[i].aabb_min[2]; const double v = dx * dy + dy * dz + dz * dx; return v == v ? (v < 1e300 ? v : 1e300) : 0.0; };      // a total order even for infinite boxes
    for (size_t k = order.size(); k-- > 0; ) {                      // children before parents
        const int j = order[k], l = nodes[j].left_or_first;
        int slot[4], ns = 0;
        for (int c = l; c <= l + 1; c++) {
            if ((nodes[c].count & 0x3fffffff) > 0) slot[ns++] = c;
            else { slot[ns++] = nodes[c].left_or_first; slot[ns++] = nodes[c].left_or_first + 1; }
        }
        auto need_of = [&](const int * sl) { int nd = 0; for (int t = 0; t < ns; t++) nd = std::max(nd, (ns - 1 - t) + need[sl[t]]); return nd; };   // slot t is walked with ns-1-t siblings pending
        int nd = max_need + 1;
        if (order_mode != 0) { std::sort(slot, slot + ns, [&](int a, int b) { return area(a) > area(b); }); nd = need_of(slot); }
        if (nd > max_need - 4) { std::sort(slot, slot + ns, [&](int a, int b) { return need[a] < need[b]; }); nd = need_of(slot); }
        need[j] = nd;
        for (int s = 0; s < ns; s++) {                              // 64 B per unit of `left`, 128 B per record (left is even)
            const rtx_bvh_node & c = nodes[slot[s]];
            rtxl::packet_from_node(out.data(), (size_t)2 * l + s, c, c.left_or_first, c.count & 0x3fffffff);
            if (slot_map) (*slot_map)[(size_t)2 * l + s] = slot[s];
        }
    }
    *stack_need = need[0];
    return true;
}

// The closest-hit per-lane walk's 4-wide records (rtx_packet.h, pk_lane_phase_closest).  BottomLevelBVH::trace (BottomLevelBVH.cpp:355-396)
// tests every node once, when it is popped, against the closest distance of that moment, and pushes an inner node's children untested, far
// child first.  With nested boxes (see build_nodes_pk4: AABB::intersect is monotone under nesting in floating point) a node that passes at
// its pop has a parent that passed at its own — earlier, hence against a distance at least as large — so the test of an inner child L of
// node X can be skipped: its children LL, LR meet, at THEIR pops, exactly the closest distances they meet in the reference (no leaf is visited
// between the pop of L and the pop of its near child), pass or fail as there, and reach the same leaves in the same order provided the four
// grandchildren are taken in the order the two binary levels would take them: X's near child's near child first.  The record of inner node
// j keeps the tree's shape for that: slots 0-1 = the left child's children (or the left child itself, a leaf, in slot 0), slots 2-3 the
// right child's; the near / far axes of the two children ride in slots 0 and 2.  Half the dependent fetches per walk.
//   record (128 B, at byte offset 64 * left-child index of j): 4 x { (min.x, min.y, max.x, max.y) (min.z, max.z, first, meta) },
//   meta = leaf count (< 16) | axis of the slot's PARENT (slots 0 and 2; 0: the parent is a leaf, i.e. the slot itself) << 26 | axis of the slot node << 30
//   (rtxl::pk4c_meta); unused slots hold a point box, which never passes.  *stack_need = pending entries a lane's walk can have (bound over all visiting orders).
static bool build_nodes_pk4c(const rtx_bvh_node * nodes, int n, int tri_count, std::vector<Quad> & out, int * stack_need, std::vector<int32_t> * slot_map = nullptr) {
    if (n >= (1 << 24) || tri_count >= (1 << 24)) return false;
    auto inside = [&](int c, int p) {
        for (int a = 0; a < 3; a++) if (!(nodes[c].aabb_min[a] >= nodes[p].aabb_min[a] && nodes[c].aabb_max[a] <= nodes[p].aabb_max[a])) return false;
        return true;
    };
    std::vector<int> order, stack(1, 0);
    while (!stack.empty()) {
        const int i = stack.back(); stack.pop_back();
        const int cnt = nodes[i].count & 0x3fffffff, f = nodes[i].left_or_first;
        if (cnt > 0) { if (!rtxl::ref_fits((uint32_t)f, (uint32_t)nodes[i].count)) return false; continue; }      // work-list and stack entries pack (first, count) into one word
        if (f & 1) return false;                                   // records are addressed by left / 2
        if (!inside(f, i) || !inside(f + 1, i)) return false;      // nesting
        order.push_back(i); stack.push_back(f); stack.push_back(f + 1);
    }
    out.assign((size_t)4 * (n > 0 ? n : 1) + 8, Quad{ 0.0f, 0.0f, 0.0f, 0.0f });
    if (slot_map) slot_map->assign((size_t)2 * (n > 0 ? n : 1) + 4, -1);
    std::vector<int> need((size_t)n, 0);
    for (size_t k = order.size(); k-- > 0; ) {                      // children before parents
        const int j = order[k], l = nodes[j].left_or_first;
        int nd = 0, ns = 0;
        for (int g = 0; g < 2; g++) {
            const rtx_bvh_node & c = nodes[l + g];
            const bool leaf = (c.count & 0x3fffffff) > 0;
            const int slots = leaf ? 1 : 2;
            for (int t = 0; t < slots; t++) {
                const int si = leaf ? l + g : c.left_or_first + t, s = 2 * g + t;
                const rtx_bvh_node & sn = nodes[si];
                rtxl::packet_from_node(out.data(), (size_t)2 * l + s, sn, sn.left_or_first, (int32_t)rtxl::pk4c_meta((uint32_t)sn.count, (uint32_t)c.count, s));
                if (slot_map) (*slot_map)[(size_t)2 * l + s] = si;
                nd = std::max(nd, need[si]); ns++;
            }
        }
        need[j] = nd + ns - 1;                                      // any slot may come first, with the others pending
    }
    *stack_need = need[0];
    return true;
}

// parent[] of a refit plan from the lane layout's topology words (a refit never writes them): the parent's index, -1 for the root,
// RTX_REFIT_UNREACHABLE for a slot no traversal reaches.  The upload validated the tree: in range, no node reachable twice.
static void parent_table(const Quad * lane_nodes, int n, std::vector<int32_t> & parent) {
    parent.assign((size_t)n, RTX_REFIT_UNREACHABLE);
    parent[0] = -1;
    std::vector<int32_t> stack(1, 0);
    while (!stack.empty()) {
        const int i = stack.back(); stack.pop_back();
        const int32_t f = rtxl::word_of(lane_nodes[2 * (size_t)i].w), cw = rtxl::word_of(lane_nodes[2 * (size_t)i + 1].w);
        if ((cw & 0x3fffffff) > 0) continue;
        parent[f] = i; parent[f + 1] = i; stack.push_back(f); stack.push_back(f + 1);
    }
}

// the balanced tree of rtx_build_math.h over T triangles, all boxes zero (nested, min <= max)
static void balanced_topology(int T, std::vector<rtx_bvh_node> & nodes) {
    const int levels = rtxb::tree_levels(T);
    nodes.assign((size_t)rtxb::tree_node_count(T), rtx_bvh_node());
    memset(nodes.data(), 0, nodes.size() * sizeof(rtx_bvh_node));
    for (int d = 0; d <= levels; d++)
        for (int j = 0; j < (1 << d); j++) {
            int first;
            const int cnt = rtxb::node_range(T, d, j, &first);
            if (cnt == 0) continue;
            rtx_bvh_node & nd = nodes[rtxu::node_slot(d, j)];
            if (cnt <= RTX_BUILD_LEAF_MAX) { nd.left_or_first = first; nd.count = cnt; }
            else { nd.left_or_first = (2 << d) | (2 * j); nd.count = 0; }
        }
}
