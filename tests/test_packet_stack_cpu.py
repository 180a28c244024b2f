"""Conditions on the INPUTS of tests/test_gpu_packet_stack.py: scenes in which the TLAS and a mesh are both deep (tests/stackset.py), the
figures the host's packet-stack rule reads from them, and what a numpy replay of the packet kernels' shared closest-hit walk has pending
on them.  Nothing here runs on a GPU and no device value is compared with the model: it only shows that the scenes sit where the rule
(plan_stack_limits, csrc/rtx_plan.h; pinned as arithmetic by csrc/plan_check.cpp) is tight.

What the model found (block (1, 1) of the tile, the grid of stackset.grid()):
  camera (a), rest of both chains on the left: sp reaches c + 1 = (n - 1) + (m - 1) + 3 — one far sibling per inner ancestor of the
      deepest leaf of either tree (dt = n - 1 in the TLAS, m - 1 in the mesh), two parked sign-split entries in the TLAS (d.y and d.z are
      mixed, d.x is not) and one more in the last instance, whose eighth turn mixes what the TLAS sorted.  The iterator entry of a
      one-instance leaf is popped when the instance is entered and is not among them; where the deepest leaf holds two instances
      (stackset.PAIR_LEAF) it stays below the BLAS part of the first.  c = 64 gives 65 entries, c = 66 gives 67: more than RTX_PK_STACK, on
      scenes the rule of the shadow-ray walk (c <= 64, or less with 4-wide records) leaves to the packet kernels.  On an MI355X exactly
      these scenes ended in RTX_ERR_LIMIT where whole packets walk everything (tests/test_gpu_packet_stack.py), so the rule now also
      bounds the shared walk (plan_shared_walk_need: dt + 3 + 1 + (m - 1) + 3 = c + 5 for two chains, the iterator entry and a third park
      per tree always counted) and sends what exceeds it to the per-lane kernels.
  camera (c), no sign disagrees: at most c - 2.
  camera (d): two lanes walk the last instance alone; with m >= 49 they want nodes with more than 46 entries of the instance pending.
"""
import numpy as np
import pytest

import stackset as S

GRID = S.grid()
IDS = [g.name for g in GRID]
ALL = S.all_scenes()
ALL_IDS = [g.name for g in ALL]


def test_grid_covers_the_bounds_in_three_splits_and_both_sides():
    assert len(GRID) == 40 and len(set(IDS)) == 40
    for c in S.GRID_C:
        for split in ("tlas", "even", "mesh"):
            sides = sorted(g.rest_left for g in GRID if g.c == c and g.split == split and g.axes == S.AXES_CYCLE)
            assert sides == [False, True], (c, split)
    assert all(8 <= g.n <= 31 and 2 <= g.m <= 57 and g.n + g.m == g.c for g in GRID)
    assert {g.n for g in GRID if g.split == "tlas"} == {31} and {g.n for g in GRID if g.split == "mesh"} == {8, 9}
    assert {g.axes for g in GRID} == {S.AXES_CYCLE, 1, 2, 3}


@pytest.mark.parametrize("g", ALL, ids=ALL_IDS)
def test_figures_follow_n_and_m(g):
    """stack_figures (csrc/rtx_api.hip) from the arrays: dt = n - 1 levels, the binary walk's blas_any = inner depth + 2 = m, blas_shared =
    2 m; both trees legal for BVH_TRAVERSAL_STACK_SIZE 64 (inner depth + 2 <= 64), so the reference overflows neither of its stacks."""
    sc = S.scene_of(g)
    f = S.figures(sc)
    assert (f.tlas_inner_depth, f.blas_inner_depth) == (g.n - 2, g.m - 2)
    assert (f.dt, f.blas_any, f.blas_shared) == (g.n - 1, g.m, 2 * g.m)
    assert f.dt + 1 + f.blas_any == g.c
    stack_size = int(sc.config["stack_size"][0])
    assert stack_size == 64 and f.tlas_inner_depth + 2 <= stack_size and f.blas_inner_depth + 2 <= stack_size
    assert S.figures(sc, pk4_need=36).blas_any == 36 and S.figures(sc, pk4_need=-1).blas_any == g.m
    assert len(sc.instances) == g.n and len(sc.blas) == 1 and len(sc.blas[0].tri_hot) == g.m
    # the chains are what they say: the rest on the chosen side, axes constant or cycling
    for nodes, k in ((sc.tlas_nodes, g.n), (sc.blas[0].nodes, g.m)):
        at = 0
        for d in range(k - 1):
            first = int(nodes[at]["left_or_first"])
            assert (int(nodes[at]["count"]) & 0x3fffffff) == 0 and int(np.uint32(nodes[at]["count"]) >> 30) == ((1 + d % 3) if g.axes == S.AXES_CYCLE else g.axes)
            rest, leaf = (first, first + 1) if g.rest_left else (first + 1, first)
            assert (int(nodes[leaf]["count"]) & 0x3fffffff) == 1 and int(nodes[leaf]["left_or_first"]) == d
            at = rest
        assert (int(nodes[at]["count"]) & 0x3fffffff) == 1 and int(nodes[at]["left_or_first"]) == k - 1
    w = sc.instances[g.n - 1]["world"].reshape(4, 4)
    assert abs(w[1, 1]) > 0.5 and abs(w[1, 2]) > 0.5                  # the last instance's turn mixes y and z


@pytest.mark.parametrize("g", ALL, ids=ALL_IDS)
def test_cameras_do_what_they_are_for(g):
    """(a) / (b): block (1, 1) has both signs of d.y and of d.z and one sign of d.x; (c): one direction; (d): in the model space of the last
    instance exactly two lanes of the block pass the mesh's root box."""
    sc = S.scene_of(g)
    for direction in (+1, -1):
        r = S.camera_block_rays(S.camera_along(g.n, g.m, direction))
        assert (np.sign(r[:, 3]) == direction).all()
        for a in (4, 5):
            assert (r[:, a] > 0).sum() == 32 and (r[:, a] < 0).sum() == 32
    r = S.block_rays(S.rays_parallel(g.n, g.m, S.deep_sign(g)))
    assert (r[:, 3:6] == r[0, 3:6]).all() and (np.sign(r[0, 3:6]) == S.deep_sign(g)).all()
    r = S.block_rays(S.rays_silhouette(sc, S.deep_sign(g)))
    w = sc.instances[g.n - 1]["world_inv"].astype(np.float64).reshape(4, 4)
    o = r[:, :3] @ w[:3, :3].T + w[:3, 3]; d = r[:, 3:6] @ w[:3, :3].T
    root = sc.blas[0].nodes[0]
    passes = S._slab(root["aabb_min"].astype(np.float64), root["aabb_max"].astype(np.float64), o, 1.0 / d, np.full(64, np.inf))
    assert passes.sum() == 2 and (np.sign(d) == S.deep_sign(g)).all()


def test_model_counts_a_hand_made_walk():
    """The replay on trees small enough to count by hand: one instance of a 4-triangle chain, rest on the left, constant axis x, rays
    along +x through every box.  TLAS: a single leaf (the iterator entry: 1, popped on entry).  BLAS: three inner nodes, each pushes its leaf
    sibling while the rest is walked first: 3 pending, no parks."""
    sc = S.two_chains(1, 4, True, True, 1)
    hw = S.packet_stack_high_water(sc, S.block_rays(S.rays_parallel(1, 4, +1)))
    assert (hw.sp, hw.rel, hw.steps) == (3, 3, 3)
    hw = S.packet_stack_high_water(sc, S.block_rays(S.rays_parallel(1, 4, -1)))      # the leaf first at every node: its sibling waits, alone
    assert (hw.sp, hw.rel) == (1, 1)
    sc = S.two_chains(3, 4, True, True, 1)          # three instances: two far siblings in the TLAS below the three of the mesh
    hw = S.packet_stack_high_water(sc, S.block_rays(S.rays_parallel(3, 4, +1)))
    assert (hw.sp, hw.rel) == (5, 3)
    hw = S.packet_stack_high_water(sc, S.camera_block_rays(S.camera_along(3, 4, +1)), ordered=False)      # BVH_TRAVERSE_TREE_NAIVE: left first, nothing parks
    assert (hw.sp, hw.rel) == (5, 3)


def test_model_high_water_marks_sit_on_both_sides_of_the_stack():
    top = {g.name: max(S.marks(g)[k].sp for k in "abcd") for g in GRID}
    for g in GRID:
        print(g.name, {k: tuple(S.marks(g)[k]) for k in "abcd"})
    assert any(v <= 58 for v in top.values())
    assert any(59 <= v <= 64 for v in top.values())
    # the reading of the walk is right: legal scenes the shadow-ray rule leaves to the packets (c <= 64) need more than the stack holds
    over = sorted(g.name for g in GRID if g.c <= 64 and S.marks(g)["a"].sp > S.PK_STACK)
    assert over == ["c64-even-L", "c64-mesh-L", "c64-tlas-L"], over
    assert max(top.values()) == 67 and {g.c for g in GRID if top[g.name] == 67} == {66}
    for g in GRID:
        if g.rest_left and g.axes == S.AXES_CYCLE:
            assert S.marks(g)["a"].sp == g.c + 1, g.name
        assert S.marks(g)["c"].sp <= (g.n - 1) + 1 + (g.m - 1), g.name          # no sign disagrees: dt + 1 + (m - 1)
        assert S.marks(g)["c"].sp <= g.c - 2
        # the host's bound on the shared walk covers every mark; where it exceeds the stack the call takes the per-lane kernels, whose one
        # stack per lane holds far siblings only: dt + (inner depth + 1) entries, which must fit RTX_MAX_STACK = 64 for the grid to be renderable
        assert top[g.name] <= S.shared_walk_bound(g.n, g.m) == g.c + 5, g.name
        f = S.figures(S.scene_of(g))
        assert f.dt + (f.blas_inner_depth + 1) == g.c - 2 and f.dt + (f.blas_inner_depth + 1) <= 64, g.name
    assert all(S.shared_walk_bound(g.n, g.m) > S.PK_STACK for g in GRID if top[g.name] > S.PK_STACK)
    for g in S.bound_scenes():                                             # the deepest two chains left to the packet kernels: the bound is 64, the marks below it
        assert S.shared_walk_bound(g.n, g.m) == S.PK_STACK and max(S.marks(g)[k].sp for k in "abcd") == (60 if g.rest_left else 57), g.name
    for name, (n, m) in S.PAIR_LEAF.items():                               # the deepest leaf holds two instances: the iterator entry is pending, and counted
        sc = S.pair_leaf_scene(name)
        f = S.figures(sc)
        assert (f.dt, f.blas_inner_depth) == (n - 2, m - 2) and int((sc.tlas_nodes["count"] & 0x3fffffff).max()) == 2 and len(sc.instances) == n
        assert S.shared_walk_bound(n, m, pair_leaf=True) == f.dt + 3 + 1 + (m - 1) + 3 == {"pair-29": 64, "pair-30": 65}[name]
        hw = S.packet_stack_high_water(sc, S.camera_block_rays(S.camera_along(n, m, +1)))
        assert hw.sp == f.dt + 2 + 1 + (m - 1) <= S.shared_walk_bound(n, m, pair_leaf=True), (name, hw)      # siblings, two TLAS parks, the iterator, the mesh's siblings


def test_silhouette_lanes_want_nodes_past_the_work_list_bound():
    """A lane turns private only while (sp - floor_sp) + 2 <= RTX_PK_FIFO: with more than 46 entries of the instance pending, a node that
    one to four lanes want stays with the packet.  Camera (d) reaches that on every mesh-heavy scene."""
    fifo = sorted(g.name for g in ALL if S.marks(g)["d"].few_rel > S.PK_FIFO - 2)
    assert len(fifo) >= 3 and set(fifo) == {g.name for g in ALL if g.split == "mesh"}, fifo
    assert set(S.FIFO_SCENES) <= set(fifo) and all(S.shared_walk_bound(S.by_name(x).n, S.by_name(x).m) <= S.PK_STACK for x in S.FIFO_SCENES)
    for name in S.FIFO_SCENES:
        assert S.marks(S.by_name(name))["d"].few_rel == S.by_name(name).m - 1


@pytest.mark.parametrize("g", ALL, ids=ALL_IDS)
def test_oracle_renders_every_scene_with_reflection_and_shadow_rays(g):
    sc = S.scene_of(g)
    assert (sc.width, sc.height, sc.tile_count) == (32, 32, 1)
    ref = S.oracle_frame(g, "a")
    assert ref["stats"]["primary"] == 1024 and ref["stats"]["reflection"] >= 1 and ref["stats"]["shadow"] >= 1
    assert np.isfinite(ref["rgb"]).all() and len(np.unique(ref["packed"])) > 8      # a picture, not one colour
