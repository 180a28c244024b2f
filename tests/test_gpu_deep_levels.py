"""The render path at its documented limit: RTX_MAX_LEVELS = 12 levels (bounces 11), levels that grow with depth, a level that is exactly
full, 33 lights, multi-batch frames at 12 levels — on the scenes of tests/deepset.py, whose properties tests/test_deep_levels_cpu.py asserts.

Every comparison is bit for bit against the oracle's frame (rgb as util.bit_exact, packed, the four ray counts), and every frame is read
through rtx_get_stats, which answers RTX_ERR_LIMIT after a queue or stack overflow (Renderer.stats raises).  What is covered:
  * every launch shape (test_gpu_parity.MODES, simple_trace, count_work with its work counters) on `shells`: packets at all 12 levels;
  * every MODES entry on `hall`: two instances, so levels 2 .. 11 take the per-lane kernels by default;
  * each of the levels 6 .. 10 as the LAST one (it spawns nothing; the merged shadow-ray launch ends there);
  * fused shading (RTX_FUSE_SHADE=1: child slots in wave-private 64-slot chunks) with level 1 exactly full, and RTX_PK_LPT=1;
  * frames of 3 x 2 tiles (right column and bottom row clipped) in six batches, three batches and one;
  * 33 lights (shadow slot = shadow_base[d] + light * level_cap[d] + rank), also across batches;
  * rtx_render_views, rtx_render_rays, an AOV call, the tile-major group path, hipGraph replay;
  * the launches one call queues at 12 levels, and at one level when no material spawns a ray;
  * the limit: bounces 11 creates a context, bounces 12 is RTX_ERR_LIMIT.
At 12 levels a tile's queues take about 0.9 GB (1.4 GB with 33 lights): every Renderer here is closed before the next one is made.
"""
import collections

import numpy as np
import pytest

import deepset
import util
from test_gpu_parity import MODES          # every launch shape rtx_render_tiles knows

pytestmark = pytest.mark.gpu

STATS = ("primary", "shadow", "reflection", "refraction")
WORK = ("closest_rays", "any_rays", "tlas_nodes_closest", "tlas_nodes_any", "blas_nodes_closest", "blas_nodes_any", "instances_closest",
        "instances_any", "tri_tests_closest", "tri_tests_any", "shaded_hits", "sky_lookups", "texel_fetches", "rays_spawned")
SHAPES = dict(MODES, simple_trace={"simple_trace": True}, count_work={"count_work": True})
TILE_SLOTS_12 = 1024 * 4095                   # ray slots of one tile at 12 levels (plan_batch)


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def scene(name, **kw):
    return {"shells": deepset.shells, "hall": deepset.hall}[name](**kw)


def assert_oracle(out, ref, what=""):
    assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])
    assert util.bit_exact(out["rgb"], ref["rgb"]), (what, int((out["rgb"].view(np.uint32) != ref["rgb"].view(np.uint32)).any(axis=-1).sum()), "pixels differ")
    assert np.array_equal(out["packed"], ref["packed"]), what


def render(api, monkeypatch, sc, env=None, calls=1, **flags):
    """`calls` frames of sc on a context created under `env` (the knobs are read once, in rtx_create); the context is closed before returning"""
    with monkeypatch.context() as m:
        for k, v in (env or {}).items():
            m.setenv(k, str(v))
        r = api.Renderer(sc)
    try:
        return [r.render(**flags) for _ in range(calls)]
    finally:
        r.close()


# ---- every launch shape at the limit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(SHAPES))
def test_shells_at_12_levels_in_every_launch_shape(api, mode, monkeypatch):
    sc = deepset.shells()
    ref = deepset.oracle_frame(sc)
    out, = render(api, monkeypatch, sc, **SHAPES[mode])
    assert_oracle(out, ref, mode)
    if mode == "count_work":
        for k in WORK:
            assert out["work"][k] == ref["work"][k], (k, out["work"][k], ref["work"][k])


@pytest.mark.parametrize("mode", list(MODES))
def test_hall_at_12_levels_per_lane_levels(api, mode, monkeypatch):
    sc = deepset.hall()
    assert len(sc.instances) == 2               # the default plan: per-lane kernels from level 2 on
    out, = render(api, monkeypatch, sc, **MODES[mode])
    assert_oracle(out, deepset.oracle_frame(sc), mode)


@pytest.mark.parametrize("mode", ["default", "serial"])
@pytest.mark.parametrize("bounces", [6, 7, 8, 9, 10])
def test_each_level_as_the_last_one(api, bounces, mode, monkeypatch):
    sc = deepset.with_bounces(deepset.hall(), bounces)
    ref = deepset.oracle_frame(sc)
    assert ref["stats"] != deepset.oracle_frame(deepset.with_bounces(sc, bounces - 1))["stats"]      # the last level holds rays
    out, = render(api, monkeypatch, sc, **MODES[mode])
    assert_oracle(out, ref, (bounces, mode))


# ---- fused shading: chunked child slots -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "serial", "serial_cull"])
@pytest.mark.parametrize("name", ["shells", "hall"])
def test_fused_shading_at_12_levels(api, name, mode, monkeypatch):
    """shells: level 1 is exactly full (2 x 1024 rays) while every wave may hold a partly used chunk — what alloc_queues' chunk_slack is for"""
    sc = scene(name)
    out, = render(api, monkeypatch, sc, {"RTX_FUSE_SHADE": 1}, **MODES[mode])
    assert_oracle(out, deepset.oracle_frame(sc), (name, mode))


def test_longest_packets_first_at_12_levels(api, monkeypatch):
    sc = deepset.shells()
    ref = deepset.oracle_frame(sc)
    for i, out in enumerate(render(api, monkeypatch, sc, {"RTX_PK_LPT": 1}, calls=3)):      # from the second call on: sorted by the previous call's costs
        assert_oracle(out, ref, i)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
BUDGETS = {"one_tile_per_batch": 1024, "two_tiles_per_batch": 2 * TILE_SLOTS_12, "one_batch": None}


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("name", ["shells", "hall"])
def test_batches_at_12_levels(api, name, budget, monkeypatch):
    """70 x 40: 3 x 2 tiles, the right column and the bottom row clipped.  A budget of 1024 slots is below one tile's need: the floor of one
    tile per batch.  All three equal the oracle, hence each other."""
    sc = scene(name, w=70, h=40)
    assert sc.tile_count == 6
    env = {} if BUDGETS[budget] is None else {"RTX_SLOT_BUDGET": BUDGETS[budget]}
    out, = render(api, monkeypatch, sc, env)
    assert_oracle(out, deepset.oracle_frame(sc), (name, budget))


@pytest.mark.parametrize("name", ["shells", "hall"])
def test_batches_at_12_levels_fused(api, name, monkeypatch):
    sc = scene(name, w=70, h=40)
    out, = render(api, monkeypatch, sc, {"RTX_SLOT_BUDGET": 1024, "RTX_FUSE_SHADE": 1})
    assert_oracle(out, deepset.oracle_frame(sc), name)


# ---- many lights --------------------------------------------------------------------------------------------------------------------------
LIGHT_MODES = {"default": ({}, {}), "serial": ({}, {"serial": True}), "lane": ({}, {"lane_trace": True}), "no_split": ({"RTX_PK_SPLIT": 0}, {})}


@pytest.mark.parametrize("mode", list(LIGHT_MODES))
def test_33_lights_at_12_levels(api, mode, monkeypatch):
    sc = deepset.hall(lights=33)
    assert deepset.light_count(sc) == 33
    env, flags = LIGHT_MODES[mode]
    out, = render(api, monkeypatch, sc, env, **flags)
    assert_oracle(out, deepset.oracle_frame(sc), mode)


def test_33_lights_across_batches(api, monkeypatch):
    sc = deepset.hall(w=70, h=40, lights=33)
    out, = render(api, monkeypatch, sc, {"RTX_SLOT_BUDGET": 2 * TILE_SLOTS_12})
    assert_oracle(out, deepset.oracle_frame(sc))


# ---- the other entry points ---------------------------------------------------------------------------------------------------------------
def test_views_at_12_levels(api):
    from pyrtx import host
    from test_gpu_views import FOV
    sc = deepset.shells()
    inner = np.linalg.norm(sc.camera["position"][0]); outer = (0.3, 0.5, -4.0)
    assert inner < deepset.RADII[0] < np.linalg.norm(outer) < deepset.RADII[1]      # the second camera sits inside the next shell
    cams = np.array([sc.camera[0], host.camera_basis(sc.width, sc.height, FOV, outer, (0, 0, 0, 1))[0]], dtype=sc.camera.dtype)
    refs = [deepset.oracle_frame(deepset.with_camera(sc, c)) for c in cams]
    assert refs[0]["packed"].tobytes() != refs[1]["packed"].tobytes()
    r = api.Renderer(sc)
    try:
        r.set_views(cams)
        out = r.render_views()
    finally:
        r.close()
    for k, ref in enumerate(refs):
        assert util.bit_exact(out["rgb"][k], ref["rgb"]), k
        assert np.array_equal(out["packed"][k], ref["packed"]), k
    for key in STATS:
        assert out["stats"][key] == sum(ref["stats"][key] for ref in refs), key


def test_ray_views_at_12_levels(api):
    from test_gpu_ray_views import pinhole_identity
    sc = deepset.shells()
    pinhole_identity(api, sc, {})               # render_rays over the pinhole's own rays == render, AOV calls included; closes its context
    pinhole_identity(api, sc, {"serial": True})


def test_aov_call_at_12_levels(api):
    from test_gpu_ray_views import ALL, assert_same
    sc = deepset.shells()
    r = api.Renderer(deepset.with_bounces(sc, 0))
    try:
        flat = r.render_aovs(ALL)
    finally:
        r.close()
    r = api.Renderer(sc)
    try:
        deep = r.render_aovs(ALL)
    finally:
        r.close()
    assert_oracle(deep, deepset.oracle_frame(sc))                           # the frame of an AOV call is the frame
    assert_oracle(flat, deepset.oracle_frame(deepset.with_bounces(sc, 0)))
    for ch in ALL:                                                          # primary-hit channels: the depth of the recursion does not enter
        assert_same(deep[ch], flat[ch], ch)
    assert np.isfinite(deep["depth"]).all()                                 # every primary ray hits a shell


def test_group_path_at_12_levels(api):
    sc = deepset.shells(w=70, h=40)
    r = api.Renderer(sc)
    try:
        full = r.render()
    finally:
        r.close()
    assert_oracle(full, deepset.oracle_frame(sc))
    r = api.Renderer(sc)                        # a context that has rendered nothing: what its framebuffer holds came through the group path
    try:
        r.group_loopback(3)
        _, packed = r.framebuffer()
    finally:
        r.close()
    assert np.array_equal(packed, full["packed"])


@pytest.mark.parametrize("mode", ["default", "serial"])
def test_graph_replay_at_12_levels(api, mode, monkeypatch):
    sc = deepset.hall()
    ref = deepset.oracle_frame(sc)
    for i, out in enumerate(render(api, monkeypatch, sc, {"RTX_GRAPH": 1}, calls=4, **MODES[mode])):      # eager, captured, replayed twice
        assert_oracle(out, ref, (mode, i))


# ---- launch count -------------------------------------------------------------------------------------------------------------------------
NAMES = {"C": "k_trace_closest", "S": "k_shade", "A": "k_trace_any", "I": "k_trace_items", "R": "k_resolve"}
# shells: one instance, so packets at every level and the split shadow-ray walk (a k_trace_items launch after each packet launch);
# the launches of one call per mode at L levels, in queueing order (the default shape interleaves two streams: compared as counts)
LAUNCHES = {
    "serial": ({"serial": True}, lambda L: "C S " * L + "A I " + "R " * L),
    "default": ({}, lambda L: "C S A I " + "C S " * (L - 1) + ("A I " if L > 1 else "") + "R " * L),
    "serial_lane": ({"serial": True, "lane_trace": True}, lambda L: "C S " * L + "A " + "R " * L),
    "serial_simple": ({"serial": True, "simple_trace": True}, lambda L: "C S A " * L + "R " * L),
}


def timed_launches(api, sc, flags):
    r = api.Renderer(sc)
    try:
        r.render(**flags)
        r.enable_timing(True)
        out = r.render(**flags)
        names = [k for k, _ in r.kernel_times()]
        r.enable_timing(False)
    finally:
        r.close()
    return out, names


@pytest.mark.parametrize("mode", list(LAUNCHES))
def test_a_12_level_call_launches_12_levels(api, mode):
    flags, rule = LAUNCHES[mode]
    sc = deepset.shells()
    out, names = timed_launches(api, sc, flags)
    want = [NAMES[s] for s in rule(12).split()]
    print(mode, collections.Counter(names))
    assert collections.Counter(names) == collections.Counter(want), (mode, names)
    if "serial" in flags:
        assert names == want, (mode, names)
    assert_oracle(out, deepset.oracle_frame(sc), mode)


@pytest.mark.parametrize("mode", ["serial", "default"])
def test_a_scene_that_spawns_nothing_launches_one_level(api, mode):
    """every reflection and transmittance zeroed: levels >= 1 are provably empty and none of their launches is queued, whatever `bounces` says"""
    flags, rule = LAUNCHES[mode]
    sc = deepset.shells()
    sc.materials["reflection"][:] = 0.0; sc.materials["transmittance"][:] = 0.0
    assert int(sc.config["bounces"][0]) == 11
    ref = deepset.oracle_frame(sc)
    assert ref["stats"]["reflection"] == 0 and ref["stats"]["refraction"] == 0
    out, names = timed_launches(api, sc, flags)
    want = [NAMES[s] for s in rule(1).split()]
    assert collections.Counter(names) == collections.Counter(want), (mode, names)
    assert_oracle(out, ref, mode)


# ---- the limit itself ---------------------------------------------------------------------------------------------------------------------
def test_bounces_11_is_the_last_that_creates_a_context(api):
    sc = deepset.shells()
    api.Renderer(deepset.with_bounces(sc, 11), upload=False).close()
    with pytest.raises(api.RtxError) as e:
        api.Renderer(deepset.with_bounces(sc, 12), upload=False)
    assert e.value.code == 4                    # RTX_ERR_LIMIT
    r = api.Renderer(deepset.with_bounces(sc, 1))      # a later valid create works
    try:
        assert_oracle(r.render(), deepset.oracle_frame(deepset.with_bounces(sc, 1)))
    finally:
        r.close()
