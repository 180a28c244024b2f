"""The packet kernels' ONE 64-entry stack where the TLAS and a mesh are both deep (scenes, cameras and the reasoning: tests/stackset.py and
tests/test_packet_stack_cpu.py; the host rule: plan_stack_limits, csrc/rtx_plan.h).  Everything is bit for bit against the oracle: colour,
packed pixels, the four ray counts, and RTX_OK from rtx_get_stats (Renderer.render raises on any other status: RTX_ERR_LIMIT is what a
dropped push of an overflowing packet stack reports).  No tolerances, and no value is compared with the numpy model.

Before the rule bounded the shared closest-hit walk (plan_shared_walk_need), an MI355X returned RTX_ERR_LIMIT ("BVH traversal stack
overflow") from rtx_get_stats for camera (a) of the three c = 66 scenes with the rest on the left in the default mode, serial or not, with
or without RTX_RENDER_PACKET_CLOSEST, for c64-mesh-L under RTX_PK_CLOSEST_ASM=0 + RTX_PK_DEFER_PRIMARY=8, and for all nine c = 64 / 65 / 66
scenes with the rest on the left under RTX_RENDER_PACKET_STATS: exactly the scenes the numpy replay puts above 64 entries.  Now the scenes
from c = 60 on (plan_shared_walk_need = c + 5 > 64) take the per-lane kernels; the c = 59 scenes (stackset.bound_scenes) are the deepest
two chains the packet kernels keep, and stackset.PAIR_LEAF puts a two-instance leaf, whose iterator entry is really pending, on the bound.

Two things no call shows from outside, which csrc/plan_check.cpp pins instead: that RTX_RENDER_PACKET_CLOSEST is dropped beyond its bound
(the frame is the same either way: asserted here), and which kernel a ray query takes at level 1 — query_setup calls the same
plan_stack_limits, but the packet and the per-lane closest-hit kernel are both timed as "k_trace_closest" and a query has no statistics
mode; the queries are compared for their answers on both sides of the bound."""
import copy

import numpy as np
import pytest

import stackset as S
import util

pytestmark = pytest.mark.gpu
f32 = np.float32
GRID = S.all_scenes()
IDS = [g.name for g in GRID]
MODES = ({}, {"serial": True}, {"packet_closest": True}, {"lane_trace": True}, {"packet_stats": True})
C64 = [g for g in GRID if g.c in (59, 64)]                  # the deepest scenes of the packet kernels, and c = 64 (per-lane kernels)
KNOB_SCENES = [g for g in GRID if g.c in (59, 63, 64)]
KNOBS = [{"RTX_PK_CLOSEST_ASM": "0", "RTX_PK_DEFER_PRIMARY": "8"}, {"RTX_PK_DEFER_PRIMARY": "64"}, {"RTX_FUSE_SHADE": "1"}, {"RTX_PK_WIDE": "0"},
         {"RTX_PK_WIDE_CLOSEST": "0"}, {"RTX_PK_SPLIT": "0"}]
STATS = ("primary", "shadow", "reflection", "refraction")


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def same(out, ref, what):
    """Ray counts, colour bits and packed pixels of a frame (or a batch of frames) against the oracle's."""
    assert {k: out["stats"][k] for k in STATS} == {k: ref["stats"][k] for k in STATS}, what
    assert util.bit_exact(out["rgb"], ref["rgb"]), (what, "rgb", int((np.asarray(out["rgb"]).view(np.uint32) != np.asarray(ref["rgb"]).view(np.uint32)).sum()))
    assert np.array_equal(out["packed"], ref["packed"]), (what, "packed")


def render(r, what, **mode):
    try:
        return r.render(**mode)
    except Exception as e:      # RtxError: name the scene and the mode next to the status
        raise AssertionError(f"{what} {mode}: {e}") from e


_ray_frames = {}


def ray_views(g):
    """Cameras (c) and (d) of a grid scene as two ray views, and the oracle's frames of them (once per module run)."""
    import orc
    if g.name not in _ray_frames:
        sc = S.scene_of(g)
        rays = np.stack([S.rays_parallel(g.n, g.m, S.deep_sign(g)), S.rays_silhouette(sc, S.deep_sign(g))])
        o = orc.OracleScene(sc)
        _ray_frames[g.name] = (rays, [o.shade_rays(rays[v]) for v in range(2)])
    return _ray_frames[g.name]


def check_scene(api, g, modes=MODES, what=""):
    """One context per scene: camera (a) through rtx_render_tiles in every mode, camera (b) as a view, cameras (c) and (d) as ray views."""
    sc = S.scene_with_camera(g, "a")
    r = api.Renderer(sc)
    ref_a, ref_b = S.oracle_frame(g, "a"), S.oracle_frame(g, "b")
    for mode in modes:
        same(render(r, f"{what}{g.name} (a)", **mode), ref_a, (what, g.name, "a", mode))
    r.set_views(S.camera_along(g.n, g.m, -1))
    for mode in modes[:2]:
        out = r.render_views(**mode)
        same({"stats": out["stats"], "rgb": out["rgb"][0], "packed": out["packed"][0]}, ref_b, (what, g.name, "b", mode))
    rays, refs = ray_views(g)
    r.set_rays(rays)
    for v, cam in enumerate("cd"):
        out = r.render_rays(v, 1)
        same({"stats": out["stats"], "rgb": out["rgb"][0], "packed": out["packed"][0]}, refs[v], (what, g.name, cam))
    return r


# ---- 1. launch shapes, every grid scene ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GRID, ids=IDS)
def test_every_launch_shape_renders_the_oracles_frame(api, g):
    """{}, serial, packet_closest (silently dropped: 2 dt + 1 + blas_shared is beyond the stack on the whole grid), lane_trace and
    packet_stats (every level walked by whole packets, no lane ever private), bounces 2: the deep order of camera (a) where the rest of
    the chains is on the left, of camera (b) where it is on the right."""
    assert int(S.scene_of(g).config["bounces"][0]) == 2
    r = check_scene(api, g)
    need = r.debug_blas_wide(0)
    assert 0 < need <= 36 and r.debug_blas_wide_closest(0) == g.m - 1      # 4-wide records on every mesh of the grid: blas_any = pk4_need
    f = S.figures(S.scene_of(g), pk4_need=need)
    assert f.dt + 1 + f.blas_any <= min(g.c, S.PK_STACK)      # the shadow-ray bound holds on every scene: what routes them is the shared walk's
    r.close()


# ---- 2. knob variants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", KNOBS, ids=["+".join(f"{k}={v}" for k, v in kn.items()) for kn in KNOBS])
def test_walk_variants_change_nothing_at_the_bounds(api, knobs, monkeypatch):
    """The c = 63 / 64 scenes and the c = 59 scenes (two of the three work-list scenes of camera (d) are among them, the third is checked
    too) under the knob sets.  Every knob tunes the packet kernels, and the c = 63 / 64 scenes now take the per-lane kernels: on those the
    run only shows that a knob does not disturb the routing or the frame; the packet walk's variants are exercised by the c = 59 scenes
    (its bound) and c58-mesh-L.  The knob sets are those of test_closest_hit_walk_variants_change_nothing: the C++
    statement of the shared walk with a threshold of 8, no shared BLAS walk at all, fused shading, the binary shadow-ray walk, the binary
    per-lane phase, no split walk."""
    scenes = KNOB_SCENES + [S.by_name(x) for x in S.FIFO_SCENES if S.by_name(x) not in KNOB_SCENES]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for g in scenes:
        r = check_scene(api, g, modes=MODES[:2], what=f"{knobs} ")
        if knobs.get("RTX_PK_WIDE") == "0": assert r.debug_blas_wide(0) == -1
        r.close()


# ---- 3. routing ------------------------------------------------------------------------------------------------------------------------
def routed(r, ref, what):
    """(the call's launch names with per-kernel timing on, packets counted by RTX_RENDER_PACKET_STATS) of serial calls; frames checked."""
    r.render(serial=True)
    r.enable_timing(True)
    out = r.render(serial=True)
    names = [k for k, _ in r.kernel_times()]
    r.enable_timing(True)                                                  # records are kept across calls: start again
    lane = r.render(serial=True, lane_trace=True)
    lane_names = [k for k, _ in r.kernel_times()]
    r.enable_timing(False)
    stat = r.render(serial=True, packet_stats=True)
    for o in (out, lane, stat):
        same(o, ref, what)
    return names, lane_names, int(stat["work"]["pk_packets"])


def assert_packets(api, sc, packets, what):
    import orc
    r = api.Renderer(sc)
    names, lane_names, pk = routed(r, orc.OracleScene(sc).render(threads=8), what)
    levels = int(sc.config["bounces"][0]) + 1
    assert names.count("k_trace_closest") == levels and lane_names.count("k_trace_closest") == levels, (what, names)
    if packets:
        assert pk > 0, what
        if r.debug_blas_wide(0) >= 0:
            assert "k_trace_items" in names and "k_trace_items" not in lane_names, (what, names)      # the split shadow-ray walk: packets only
    else:
        assert pk == 0 and names == lane_names and "k_trace_items" not in names, (what, names, pk)      # per-lane kernels at every level and for shadow rays
    return r


def test_shared_walk_bound_routes_two_chains(api, monkeypatch):
    """plan_shared_walk_need = c + 5 for two chains: 64 (c = 59 and below) stays with the packet kernels, 66 (c = 61 and beyond, where the
    model and the device overflowed) takes the per-lane kernels at every level and for shadow rays — with 4-wide records and with the
    binary shadow-ray walk (RTX_PK_WIDE=0), whose own bound c = dt + 1 + blas_any <= 64 two chains can no longer reach first."""
    cases = (("c58-tlas-L", True), ("c59-tlas-L", True), ("c59-mesh-R", True), ("c61-tlas-L", False), ("c61-mesh-R", False), ("c64-even-L", False),
             ("c65-tlas-L", False), ("c66-mesh-L", False))
    for wide in (True, False):
        if not wide: monkeypatch.setenv("RTX_PK_WIDE", "0")
        for name, packets in cases:
            g = S.by_name(name)
            assert (S.shared_walk_bound(g.n, g.m) <= S.PK_STACK) == packets
            r = assert_packets(api, S.scene_with_camera(g, "a"), packets, f"{'wide' if wide else 'binary'} {name}")
            assert (r.debug_blas_wide(0) >= 0) == wide
            r.close()


def test_two_chains_one_past_the_bound_take_the_per_lane_kernels(api):
    """c = 60 (65 by the rule) is in no grid: 31 x 29, 21 x 39 and 8 x 52, rest on the left."""
    for n, m in ((31, 29), (21, 39), (8, 52)):
        assert S.shared_walk_bound(n, m) == 65
        assert_packets(api, S.two_chains(n, m), False, f"c=60 {n}x{m}").close()


@pytest.mark.parametrize("name", sorted(S.PAIR_LEAF))
def test_a_two_instance_leaf_at_the_bound(api, name):
    """The deepest TLAS leaf holds two instances, so its iterator entry lies below the BLAS part of the first: dt 29 over 29 triangles is
    64 by the rule (packets; the statistics mode walks everything with whole packets), over 30 it is 65 (per-lane kernels)."""
    import orc
    n, m = S.PAIR_LEAF[name]
    sc = S.pair_leaf_scene(name)
    packets = S.shared_walk_bound(n, m, pair_leaf=True) <= S.PK_STACK
    assert packets == (name == "pair-29")
    r = assert_packets(api, sc, packets, name)
    ref = orc.OracleScene(sc).render(threads=8)
    for mode in MODES:
        same(render(r, name, **mode), ref, (name, mode))
    r.close()


def test_tlas_bound_routes_by_two_dt_plus_one(api):
    """2 dt + 1 = 63 (32 instances): packets; 65 (33 instances): per-lane kernels, whatever the mesh."""
    assert_packets(api, S.two_chains(32, 4), True, "2dt+1=63").close()
    assert_packets(api, S.two_chains(33, 4), False, "2dt+1=65").close()


def test_packet_closest_is_dropped_across_the_shared_bound(api):
    """2 dt + 1 + blas_shared = 63 / 65 (dt 6; m 25 / 26): the flag holds / is dropped silently; on both sides of the level-0 bound
    (c + 5 = 64 / 65) the frame is the oracle's, flag or no flag.  That the flag is dropped shows in no frame: csrc/plan_check.cpp pins it."""
    import orc
    for n, m in ((7, 25), (7, 26), (31, 28), (31, 29)):
        sc = S.two_chains(n, m)
        ref = orc.OracleScene(sc).render(threads=8)
        r = api.Renderer(sc)
        for mode in ({"packet_closest": True}, {"packet_closest": True, "serial": True}, {}):
            same(render(r, f"n={n} m={m}", **mode), ref, (n, m, mode))
        r.close()


# ---- 4. other entry points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", C64, ids=[g.name for g in C64])
def test_views_rays_with_aovs_and_the_group_path(api, g):
    import orc
    sc = S.scene_with_camera(g, "a")
    r = api.Renderer(sc)
    r.set_views(np.concatenate([S.camera_along(g.n, g.m, +1), S.camera_along(g.n, g.m, -1)]))
    out = r.render_views()
    refs = [S.oracle_frame(g, "a"), S.oracle_frame(g, "b")]
    assert {k: out["stats"][k] for k in STATS} == {k: refs[0]["stats"][k] + refs[1]["stats"][k] for k in STATS}
    for v in range(2):
        assert util.bit_exact(out["rgb"][v], refs[v]["rgb"]) and np.array_equal(out["packed"][v], refs[v]["packed"]), (g.name, v)
    rays, ray_refs = ray_views(g)
    r.set_rays(rays[:1])
    out = r.render_rays(aovs=("depth", "object_id", "triangle_id"))
    same({"stats": out["stats"], "rgb": out["rgb"][0], "packed": out["packed"][0]}, ray_refs[0], (g.name, "c"))
    hits, ids = orc.OracleScene(sc).trace_closest(rays[0].reshape(-1, 18))
    hit = hits[:, 0] > 0
    assert hit.any()
    assert util.bit_exact(out["depth"].reshape(-1), np.where(hit, hits[:, 1], f32(np.inf)).astype(f32))
    assert np.array_equal(out["object_id"].reshape(-1).view(np.int32)[hit], ids[hit, 1]) and np.array_equal(out["triangle_id"].reshape(-1).view(np.int32)[hit], ids[hit, 2])
    r.group_loopback(2)                                                    # the tile-major group path at world 2
    assert np.array_equal(r.framebuffer()[1], refs[0]["packed"]), g.name
    r.close()


# ---- 5. ray queries --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", C64, ids=[g.name for g in C64])
def test_ray_queries_of_the_primary_rays_and_the_first_lights_shadow_segments(api, g):
    """The 1 024 primary rays of camera (a) as rows of rtx_query_closest, all channels, sorted and unsorted, and the shadow segments of
    the first light (from every hit point to the light on the row's axis) as rows of rtx_query_occluded: the oracle's batch answers."""
    import orc
    import torch
    from test_gpu_query import expected, check_channels, zero_diff
    sc = S.scene_with_camera(g, "a")
    o = orc.OracleScene(sc)
    rays = np.ascontiguousarray(api.pinhole_rays(sc.camera, S.SIZE, S.SIZE).reshape(-1, 18)[:, :6])
    want = expected(o, rays)
    hit = np.isfinite(want["distance"])
    assert hit.sum() > 64
    light = sc.point_lights["position"][0].astype(f32)
    to = light[None, :] - want["position"][hit]
    dist = np.sqrt((to * to).sum(axis=1)).astype(f32)
    seg = np.concatenate([want["position"][hit], (to / dist[:, None]).astype(f32), dist[:, None]], axis=1).astype(f32)
    occ = o.trace_any(zero_diff(seg[:, :6]), seg[:, 6])
    assert occ.any()
    r = api.Renderer(sc)
    rays_t, seg_t = torch.from_numpy(rays).cuda(), torch.from_numpy(seg).cuda()
    for kw in ({}, {"sort": True}, {"lane_trace": True}, {"packet_closest": True, "sort": True}):
        check_channels(r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), **kw), want, None, f"{g.name} {kw}")
    for kw in ({}, {"sort": True}, {"lane_trace": True}):
        got = r.query_occluded(seg_t, **kw).cpu().numpy()
        assert np.array_equal(got != 0, occ), (g.name, kw, int(((got != 0) != occ).sum()))
    same(render(r, g.name), S.oracle_frame(g, "a"), (g.name, "frame after the queries"))
    r.close()


# ---- 6. a scene across a bound between two calls ---------------------------------------------------------------------------------------
def test_set_frame_and_update_instances_move_a_context_across_the_bound(api):
    """31 instances over 28 triangles (the shared walk's bound: 64), then rtx_set_frame with one more instance (65: the next call takes the
    per-lane kernels), then back (packets again); then rtx_update_instances, whose balanced TLAS is shallow (packets whatever n).  Every
    frame is the oracle's."""
    import orc
    import torch
    n, m = 31, 28
    assert S.shared_walk_bound(n, m) == 64 and S.shared_walk_bound(n + 1, m) == 65
    small, big = S.two_chains(n, m), S.two_chains(n + 1, m)
    refs = {id(s): orc.OracleScene(s).render(threads=8) for s in (small, big)}
    r = api.Renderer(small)
    for step, (sc, packets) in enumerate(((small, True), (big, False), (small, True), (big, False))):
        if step: r.set_frame(sc)
        names, lane_names, pk = routed(r, refs[id(sc)], f"step {step}")
        assert (pk > 0) == packets and ("k_trace_items" in names) == packets and (names == lane_names) == (not packets), (step, names, pk)
    pos = np.stack([np.array([x, 0.0, 0.0], f32) for x in S.row_positions(n + 1, m)]).astype(f32)
    rot = np.array([S.rotation_of(k, n + 1) for k in range(n + 1)], f32)
    r.update_instances(torch.from_numpy(pos).cuda(), torch.from_numpy(rot).cuda())
    inst, nodes, idx = r.read_frame_state()
    now = copy.copy(big)
    now.instances, now.tlas_nodes, now.tlas_indices = inst, nodes, idx
    assert S.inner_depth(nodes) + 2 + 36 <= 64
    names, lane_names, pk = routed(r, orc.OracleScene(now).render(threads=8), "after update_instances")
    assert pk > 0 and "k_trace_items" in names
    r.close()
