"""The persistent render kernels past their static first round.

Every traversal kernel of the render path is a persistent grid sized from the device (csrc/rtx_api.hip rtx_create: compute units x occupancy):
round one is static (thread or wave w takes ray or packet w), the later rounds are dynamic — k_packet fetches from eight atomic packet heads
and steals once from a neighbour class, k_trace_fast and k_trace refill single lanes through refill_index while the wave's other lanes are in
mid-walk, k_items takes units round-robin.  On a device of hundreds of compute units the 320 x 180 frames the rest of the suite renders end
inside round one.  Here RTX_GRID_CUS sizes the grids for one compute unit (two, three), so the same small frames go through many dynamic
rounds, and Renderer.debug_grids() — what the library really launches — is read in every case to assert that they do:
    primary slots >= 4 x threads of the per-lane / plain grids,   primary slots / 64 >= 4 x waves of the packet grids.
References are the ones the suite trusts already: the reference-made goldens of tests/golden (frames bit for bit, packed pixels, the four ray
counts) and the oracle (work counters, dynamic scenes, cameras, queries, AOVs); never a default-grid context of the same library alone.
Two wrong builds, tried on an MI355X and not kept: the plain kernel's step count not reset at a refill fails both heat-map cases here and
none of the default-grid heat-map tests; packet heads armed at 0 instead of waves / 8 hands the first round's packets out again, which no
frame shows outside the fused kernel (a packet traced twice writes the same hits) — the packet_stats cases count the packets walked.
"""
import numpy as np
import pytest

import util
from test_gpu_parity import MODES          # every launch shape rtx_render_tiles knows

pytestmark = pytest.mark.gpu
f32 = np.float32

CUS, TRACE_CLOSEST, TRACE_ANY, TRACE_COUNT, PK_CLOSEST, PK_ANY, ITEMS, SPILL = range(8)      # Renderer.GRID_NAMES
TRACE_BLOCK, WAVE = 256, 64                                                                   # RTX_TRACE_BLOCK; one wave per packet / item workgroup
SHAPES = dict(MODES, count_work={"count_work": True}, simple_trace={"simple_trace": True}, packet_stats={"packet_stats": True})
ALL_KINDS = ("lane", "plain", "packet")
WORK_KEYS = ("closest_rays", "any_rays", "tlas_nodes_closest", "tlas_nodes_any", "blas_nodes_closest", "blas_nodes_any", "instances_closest",
             "instances_any", "tri_tests_closest", "tri_tests_any", "shaded_hits", "sky_lookups", "texel_fetches", "rays_spawned")
RATIOS = {}                                # kind -> the smallest units-per-thread / packets-per-wave ratio a case ran at (printed by each case)


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def renderer(api, monkeypatch, sc, cus=1, **knobs):
    """A fresh context sized for `cus` compute units (None: the device's): the knobs are read once, in rtx_create."""
    if cus is None:
        monkeypatch.delenv("RTX_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("RTX_GRID_CUS", str(cus))
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    r = api.Renderer(sc)
    for k in knobs:
        monkeypatch.delenv(k)
    if cus is not None:
        assert r.debug_grids()[CUS] == cus
    return r


def past_first_round(r, slots, kinds=ALL_KINDS, what=""):
    """The non-vacuity condition, from the grids the context launches: `slots` primary slots of a batch are at least four rounds of every
    grid named.  lane / plain: the per-lane / plain kernels (a ray per thread); packet: the packet kernels (a 64-slot packet per wave)."""
    g = [int(v) for v in r.debug_grids()]
    assert min(g) >= 1, g
    assert g[SPILL] >= TRACE_BLOCK * max(g[TRACE_CLOSEST], g[TRACE_ANY], g[TRACE_COUNT]) and g[SPILL] >= WAVE * max(g[PK_CLOSEST], g[PK_ANY]), g
    assert g[PK_CLOSEST] % 8 == 0 and g[PK_ANY] % 8 == 0, g              # whole rounds of the eight packet heads
    units = {"lane": (slots, TRACE_BLOCK * max(g[TRACE_CLOSEST], g[TRACE_ANY])), "plain": (slots, TRACE_BLOCK * g[TRACE_COUNT]),
             "packet": (slots // 64, max(g[PK_CLOSEST], g[PK_ANY])), "packet_closest": (slots // 64, g[PK_CLOSEST]),
             "packet_any": (slots // 64, g[PK_ANY])}
    for kind in kinds:
        have, grid = units[kind]
        assert have >= 4 * grid, (what, kind, have, grid, g)
        RATIOS[kind] = min(RATIOS.get(kind, 1e30), have / grid)
    print(f"grids {what}: {g}, {slots} slots, rounds " + ", ".join(f"{k} {units[k][0] / units[k][1]:.1f}" for k in kinds)
          + "; smallest so far " + ", ".join(f"{k} {v:.1f}" for k, v in RATIOS.items()))
    return g


def assert_golden(out, g, what=""):
    cmp = util.compare_to_golden(out, g)
    assert cmp["stats_equal"], (what, out["stats"], g["stats"].tolist())
    assert cmp["nan_mismatch"] == 0 and cmp["max_abs"] == 0.0 and cmp["n_diff_pixels"] == 0, (what, cmp)      # identical; a NaN equals a NaN
    assert cmp["packed_mismatch"] == 0, (what, cmp)


def assert_same_frame(out, ref, what=""):
    assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])
    assert util.bit_exact(out["rgb"], ref["rgb"]), what
    assert np.array_equal(out["packed"], ref["packed"]), what


_ORACLE = {}


def oracle_frame(key, sc):
    """The oracle's frame, ray counts and work counters of a scene, once per run."""
    if key not in _ORACLE:
        import orc
        _ORACLE[key] = orc.OracleScene(sc).render(threads=8)
    return _ORACLE[key]


_PACKETS = {}


def packets_walked_once(api, monkeypatch, name, sc):
    """Packets of a packet_stats frame on the device's own grids, where no launch of a 320 x 180 frame leaves the static round (wave w takes
    packet w, once, by construction): the count itself is no reference for pixels, only for how often the queue hands a packet out."""
    if name not in _PACKETS:
        r = renderer(api, monkeypatch, sc, None)
        g = [int(v) for v in r.debug_grids()]
        assert min(g[PK_CLOSEST], g[PK_ANY]) >= sc.tile_count * 16 * 2, g      # room for level 0's packets and its shadow rays' per light
        _PACKETS[name] = r.render(packet_stats=True)["work"]["pk_packets"]
        r.close()
    return _PACKETS[name]


# ---- 1. launch shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ["materials_aniso", "tori16", "monkey_small", "coincident", "materials_b5", "materials_naive"])
def test_every_launch_shape_on_one_compute_unit(api, monkeypatch, name, shape):
    """Each context renders twice: the second frame meets the heads and counters the first one used."""
    sc, g = util.load_golden(name)
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, sc.tile_count * 1024, what=f"{name} {shape}")
    for frame in range(2):
        out = r.render(**SHAPES[shape])
        assert_golden(out, g, f"{name} {shape} frame {frame}")
        if shape == "count_work":
            ref = oracle_frame(name, sc)
            bad = {k: (out["work"][k], ref["work"][k]) for k in WORK_KEYS if out["work"][k] != ref["work"][k]}
            assert not bad, (name, frame, bad)
        if shape == "packet_stats":                                    # every packet walked exactly once: a head that starts too early hands packets out again
            assert out["work"]["pk_packets"] == packets_walked_once(api, monkeypatch, name, sc) >= sc.tile_count * 16, (name, frame)
    r.close()


@pytest.mark.parametrize("name", ["monkey_small_heat", "materials_heat"])
def test_heat_maps_on_one_compute_unit(api, monkeypatch, name):
    """The plain kernel's per-ray step count is the pixel: a lane that kept its previous ray's count after a refill shows."""
    sc, g = util.load_golden(name)
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, sc.tile_count * 1024, ("plain",), name)
    for frame in range(2):
        assert_golden(r.render(), g, f"{name} frame {frame}")
        counted = r.render(count_work=True)
        assert_golden(counted, g, f"{name} frame {frame} count_work")
        assert counted["work"]["closest_rays"] == sc.width * sc.height
    r.close()


@pytest.mark.parametrize("shape", ["default", "serial", "lane"])
@pytest.mark.parametrize("cus", [2, 3])
def test_two_and_three_compute_units(api, monkeypatch, cus, shape):
    """Odd products of compute units and occupancy go through the packet grids' round-up to whole rounds of the eight heads."""
    sc, g = util.load_golden("materials_aniso")
    r = renderer(api, monkeypatch, sc, cus)
    past_first_round(r, sc.tile_count * 1024, what=f"{cus} compute units {shape}")
    for frame in range(2):
        assert_golden(r.render(**SHAPES[shape]), g, f"{cus} compute units {shape} frame {frame}")
    r.close()


# ---- 2. the grid knobs there were, on the whole device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,name,kind", [("RTX_PK_GRID_CLOSEST", "materials_aniso", "packet_closest"), ("RTX_PK_GRID_ANY", "materials_aniso", "packet_any"),
                                            ("RTX_PK_GRID_SCALE", "materials_aniso", "packet_closest"), ("RTX_PK_GRID_SCALE", "cube", "packet"),
                                            ("RTX_ITEM_GRID", "materials_aniso", None)])
def test_grid_knobs_on_the_whole_device(api, monkeypatch, knob, name, kind):
    """0.05 workgroups per compute unit (RTX_PK_GRID_SCALE: 0.05 of the occupancy-sized grid): the read-back shows the grid asked for, whole
    rounds of eight for the packet grids, and the frame is the reference's in both launch shapes.  A twentieth of the occupancy-sized
    shadow-ray grid still holds more than a quarter of the 960 packets of a 320 x 180 frame, so under RTX_PK_GRID_SCALE that frame stands
    for the closest-hit grid alone, and the 1 024 packets of the 256 x 256 cube for both."""
    sc, g = util.load_golden(name)
    base = [int(v) for v in renderer(api, monkeypatch, sc, None).debug_grids()]
    r = renderer(api, monkeypatch, sc, None, **{knob: "0.05"})
    grids = [int(v) for v in r.debug_grids()]
    cu = base[CUS]
    rounded = lambda x: max((((int(x) + 1) & ~1) + 7) // 8 * 8, 8)
    want = list(base)
    if knob == "RTX_PK_GRID_CLOSEST":
        want[PK_CLOSEST] = rounded(cu * 0.05)
    elif knob == "RTX_PK_GRID_ANY":
        want[PK_ANY] = rounded(cu * 0.05)
    elif knob == "RTX_PK_GRID_SCALE":
        want[PK_CLOSEST] = rounded(base[PK_CLOSEST] * 0.05); want[PK_ANY] = rounded(base[PK_ANY] * 0.05)
    else:
        want[ITEMS] = max(int(cu * 0.05), 1)
    assert grids[:SPILL] == want[:SPILL], (knob, grids, want, base)
    assert grids[SPILL] <= base[SPILL]
    if kind:
        past_first_round(r, sc.tile_count * 1024, (kind,), f"{knob} {name}")
    else:
        assert grids[ITEMS] * 16 <= base[ITEMS], (grids, base)
    for shape in ("default", "serial"):
        for frame in range(2):
            assert_golden(r.render(**SHAPES[shape]), g, f"{knob} {shape} frame {frame}")
    r.close()


# ---- 3. knob combinations under the small grid ------------------------------------------------------------------------------------------
COMBOS = {
    "fused_shade": ({"RTX_FUSE_SHADE": "1"}, {}),
    "fused_shade_cull": ({"RTX_FUSE_SHADE": "1"}, {"cull_dead_shadow_rays": True}),
    "no_split": ({"RTX_PK_SPLIT": "0"}, {}),
    "item_chunks_fill": ({"RTX_PK_ITEM_BYTES": "per wave 64"}, {}),
    "one_item_workgroup": ({"RTX_ITEM_GRID": "0.05"}, {}),
    "lane_from_0": ({"RTX_LANE_FROM_LEVEL": "0"}, {}),
    "lane_from_1": ({"RTX_LANE_FROM_LEVEL": "1"}, {}),
    "no_pk_order": ({"RTX_PK_ORDER": "0"}, {}),
    "pk4_stack_order": ({"RTX_PK4_ORDER": "0"}, {}),
    "binary_shadow_walk": ({"RTX_PK_WIDE": "0"}, {}),
    "binary_private_walk": ({"RTX_PK_WIDE_CLOSEST": "0"}, {}),
    "compiled_shared_walk": ({"RTX_PK_CLOSEST_ASM": "0"}, {}),
    "resolve_block_64": ({"RTX_RESOLVE_BLOCK": "64"}, {}),
}


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("name", ["materials_aniso", "tori16"])
def test_knob_combinations_on_one_compute_unit(api, monkeypatch, name, combo):
    knobs, extra = COMBOS[combo]
    knobs = dict(knobs)
    sc, g = util.load_golden(name)
    if combo == "item_chunks_fill":                                    # the item buffer bounded to 64 items (one unit) per wave of the shadow-ray launch
        probe = renderer(api, monkeypatch, sc)
        knobs["RTX_PK_ITEM_BYTES"] = str(int(probe.debug_grids()[PK_ANY]) * 64 * 48)
        probe.close()
    r = renderer(api, monkeypatch, sc, 1, **knobs)
    grids = past_first_round(r, sc.tile_count * 1024, what=f"{name} {combo}")
    if combo == "one_item_workgroup":
        assert grids[ITEMS] == 1
    for shape in ("default", "serial"):
        for frame in range(2):
            assert_golden(r.render(**dict(SHAPES[shape], **extra)), g, f"{name} {combo} {shape} frame {frame}")
    r.close()


@pytest.mark.parametrize("lpt", ["-1", "1", "0"])
def test_longest_packets_first_on_one_compute_unit(api, monkeypatch, lpt):
    """A series of four frames per shape, then the two half tile ranges, as test_gpu_parity.test_longest_packets_first_changes_nothing does.
    With -1 the default rule (csrc/rtx_plan.h: the two-stream shape and at least two packets per wave; pinned by plan_check) is now on:
    its condition is asserted from the grid read back."""
    sc, g = util.load_golden("materials_aniso")
    r = renderer(api, monkeypatch, sc, 1, RTX_PK_LPT=lpt)
    grids = past_first_round(r, sc.tile_count * 1024, ("packet_closest",), f"lpt {lpt}")
    half = sc.tile_count // 2
    assert sc.tile_count * 16 >= 2 * grids[PK_CLOSEST] and half * 16 >= 2 * grids[PK_CLOSEST]      # the rule holds for the frame and for each half
    for shape in ("default", "serial", "default"):
        for frame in range(4):
            assert_golden(r.render(**SHAPES[shape]), g, f"lpt {lpt} {shape} frame {frame}")
    for frame in range(3):
        r.render_async(0, 1, half)
    for frame in range(3):
        r.render_async(half, 1, sc.tile_count - half)
    r.synchronize()
    _, packed = r.framebuffer()
    assert np.array_equal(packed, np.asarray(g["packed"]).reshape(packed.shape))
    r.close()


@pytest.mark.parametrize("shape", ["default", "serial", "lane", "count_work"])
def test_several_batches_per_call(api, monkeypatch, shape):
    """20 tiles per batch, three batches: k_begin_batch re-arms the heads and the fetch counters each time."""
    sc, g = util.load_golden("materials_aniso")
    assert sc.tile_count == 60 and int(sc.config["bounces"][0]) == 3
    r = renderer(api, monkeypatch, sc, 1, RTX_SLOT_BUDGET=1024 * 15 * 20)
    past_first_round(r, 20 * 1024, what=f"batches {shape}")
    for frame in range(2):
        assert_golden(r.render(**SHAPES[shape]), g, f"three batches {shape} frame {frame}")
    r.close()


def test_graph_replay_on_one_compute_unit(api, monkeypatch):
    """An eager call, the capture, three replays; a changed call; and the same again."""
    sc, g = util.load_golden("materials_aniso")
    r = renderer(api, monkeypatch, sc, 1, RTX_GRAPH=1)
    past_first_round(r, sc.tile_count * 1024, what="graph")
    for series in range(2):
        for call in range(5):
            assert_golden(r.render(), g, f"series {series} call {call}")
        assert_golden(r.render(serial=True, cull_dead_shadow_rays=True), g, f"series {series}, the changed call")
    r.close()


# ---- 4. views, ray views, AOVs ----------------------------------------------------------------------------------------------------------
VIEWS = (0, 2, 3)                          # of test_gpu_views.camera_set: a moved camera, the scene's own, an axis-aligned one


def view_cameras(sc):
    from test_gpu_views import camera_set
    return camera_set(sc)[list(VIEWS)]


def check_aovs(out, k, key, sc):
    """View k's channels against the oracle's trace of the camera's primary rays, as test_gpu_aov.test_channels_match_the_oracle does."""
    import test_gpu_aov as A
    dist, rays, hits, albedo, ids = A.oracle(key, sc)
    one = {ch: out[ch][k] for ch in A.ALL}
    hit = hits[:, 0] > 0
    assert hit.any()
    A.assert_same(A.flat(one, "depth"), dist, "depth")
    A.assert_same(A.flat(one, "position")[hit], hits[hit, 2:5], "position")
    A.assert_same(A.flat(one, "normal")[hit], hits[hit, 5:8], "normal")
    A.assert_same(A.flat(one, "uv")[hit], hits[hit, 9:11], "uv")
    A.assert_same(A.flat(one, "albedo"), albedo, "albedo")
    for ch in ("position", "normal", "uv"):
        assert not A.flat(one, ch)[~hit].any(), ch
    for j, ch in enumerate(A.IDS):
        A.assert_same(A.flat(one, ch), ids[:, j], ch)


@pytest.mark.parametrize("shape", ["default", "serial", "lane"])
@pytest.mark.parametrize("call", ["views", "rays"])
def test_views_and_ray_views_with_every_channel(api, monkeypatch, call, shape):
    """Three cameras of materials_aniso in one call, as cameras and as caller rays: every view is the oracle's frame of its camera, the ray
    counts are the sum, every AOV channel is the oracle's."""
    import test_gpu_aov as A
    from test_gpu_views import with_camera
    sc, g = util.load_golden("materials_aniso")
    cams = view_cameras(sc)
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, sc.tile_count * 1024, what=f"{call} {shape}")
    if call == "views":
        r.set_views(cams)
    else:
        r.set_rays(np.stack([api.pinhole_rays(c, sc.width, sc.height) for c in cams]))
    for frame in range(2):
        out = (r.render_views if call == "views" else r.render_rays)(aovs=A.ALL, **SHAPES[shape])
        refs = []
        for k, v in enumerate(VIEWS):
            cam_sc = with_camera(sc, cams[k])
            ref = oracle_frame(("materials_aniso view", v), cam_sc)
            refs.append(ref)
            assert util.bit_exact(out["rgb"][k], ref["rgb"]) and np.array_equal(out["packed"][k], ref["packed"]), (call, shape, frame, v)
            check_aovs(out, k, "materials_aniso" if v == 2 else f"materials_aniso view {v}", cam_sc)
        for key in ("primary", "shadow", "reflection", "refraction"):
            assert out["stats"][key] == sum(ref["stats"][key] for ref in refs), (key, out["stats"])
    assert_golden({"rgb": out["rgb"][1], "packed": out["packed"][1], "stats": refs[1]["stats"]}, g, "the scene's own camera")
    r.close()


# ---- 5. frames after device-side changes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["default", "serial", "lane"])
def test_frame_after_update_instances(api, monkeypatch, shape):
    import test_gpu_update_instances as U
    from test_tlas_balanced_cpu import poses
    sc, _ = util.load_golden("tori16")
    pos, rot = poses("tori16", 3)
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, sc.tile_count * 1024, what=f"update {shape}")
    r.render(**SHAPES[shape])                                            # a frame of the uploaded state first
    p, q = U.dev(pos), U.dev(rot)
    r.update_instances(p, q)
    state = r.read_frame_state()
    U.assert_state(state, U.host_state(sc, pos, rot))
    for frame in range(2):
        assert_same_frame(r.render(**SHAPES[shape]), U.oracle_frame(sc, state, "tori16_f3"), f"after the update, {shape} frame {frame}")
    r.close()


@pytest.mark.parametrize("shape", ["default", "serial", "lane"])
def test_frame_after_refit_blas(api, monkeypatch, shape):
    import test_gpu_blas_refit as R
    from test_blas_refit_cpu import FRAME_CASES
    from test_tlas_balanced_cpu import poses
    kind, seed, amp = FRAME_CASES[0]
    sc, sv, verts, twin = R.refit_case(kind, seed, amp, "golden")
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, sc.tile_count * 1024, what=f"refit {shape}")
    r.bind_blas_vertices(0, sv, len(verts))
    assert_same_frame(r.render(**SHAPES[shape]), R.oracle_frame(sc, ("base", "golden")), f"before the refit, {shape}")
    pos, rot = poses("tori16", 1)
    v, p, q = R.dev(verts), R.dev(pos), R.dev(rot)
    r.refit_blas(0, v)
    r.update_instances(p, q)
    for frame in range(2):
        assert_same_frame(r.render(**SHAPES[shape]), R.oracle_frame(twin, (kind, "golden")), f"after the refit, {shape} frame {frame}")
    r.close()


@pytest.mark.parametrize("shape", ["default", "serial", "lane"])
def test_frame_after_build_blas(api, monkeypatch, shape):
    """The Torus with padded invalid triangles, deformed, built on the device under the 16 instances of tori16 at the golden's 320 x 180."""
    import test_gpu_blas_build as B
    from test_blas_refit_cpu import tori_scene
    from test_tlas_balanced_cpu import poses
    sc = tori_scene(B.twin_of("torus")[0])
    tw = tori_scene(B.twin_of("padded", True, 1)[0])
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, sc.tile_count * 1024, what=f"build {shape}")
    assert_same_frame(r.render(**SHAPES[shape]), oracle_frame("tori around the torus twin", sc), f"before the build, {shape}")
    keep = B.build_on_device(r, "padded", True, 1)
    pos, rot = poses("tori16", 1)
    p, q = B.dev(pos), B.dev(rot)
    r.update_instances(p, q)
    for g_, w in zip(r.read_frame_state(), (tw.instances, tw.tlas_nodes, tw.tlas_indices)):
        assert g_.tobytes() == w.tobytes()
    ref = oracle_frame("tori around the padded twin", tw)
    for frame in range(2):
        assert_same_frame(r.render(**SHAPES[shape]), ref, f"after the build, {shape} frame {frame}")
    assert not np.array_equal(ref["packed"], oracle_frame("tori around the torus twin", sc)["packed"])
    del keep
    r.close()


# ---- 6. queries --------------------------------------------------------------------------------------------------------------------------
def test_ray_queries_and_debug_hooks_on_one_compute_unit(api, monkeypatch):
    """query_closest and query_occluded with at least four rounds of every grid, sorted and unsorted, through every kernel a flag selects,
    and the two debug hooks over the same rows: the oracle's answers, bit for bit."""
    import test_gpu_query as Q
    from test_gpu_rays import LANE_TRACE, check_occ
    sc, rays, dist, labels, want, occ = Q.generated("materials_aniso", n=256, seed=22)
    r = renderer(api, monkeypatch, sc)
    g = [int(v) for v in r.debug_grids()]
    n = 4 * max(TRACE_BLOCK * max(g[TRACE_CLOSEST], g[TRACE_ANY]), WAVE * max(g[PK_CLOSEST], g[PK_ANY])) + 37
    past_first_round(r, n, ("lane", "packet"), "ray queries")
    pick = np.random.default_rng(9).integers(len(rays), size=n)
    rays, dist, occ, labels = rays[pick], dist[pick, 1:2], occ[pick, 1:2], labels[pick]      # segments: exactly at the hit, the tie the strict < decides
    want = {k: v[pick] for k, v in want.items()}
    rays_t, seg = Q.dev(rays), Q.segments_of(rays, dist)
    seg_t = Q.dev(seg)
    for sort in (False, True):
        for flags, kw in Q.FLAGS.items():
            got = r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), sort=sort, **kw)
            Q.check_channels(got, want, labels, f"closest flags {flags} sort {sort}")
        for flags in (0, LANE_TRACE):
            got = Q.host(r.query_occluded(seg_t, sort=sort, **Q.FLAGS[flags]))
            check_occ(got.reshape(dist.shape) != 0, occ, labels)
    mat = np.where(want["material_id"] < 0, 0, want["material_id"]).astype(f32)
    for flags in Q.FLAGS:
        hook = r.debug_trace_rays(Q.zero_diff(rays), flags)
        cols = {"hit": (hook[:, 0], (want["object_id"] >= 0).astype(f32)), "distance": (hook[:, 1], want["distance"]), "point": (hook[:, 2:5], want["position"]),
                "normal": (hook[:, 5:8], want["normal"]), "material_id": (hook[:, 8], mat), "u, v": (hook[:, 9:11], want["uv"])}
        bad = {k: np.flatnonzero(~Q.same_bits(a, b))[:6].tolist() for k, (a, b) in cols.items() if not Q.same_bits(a, b).all()}
        assert not bad, (flags, bad)
    for flags in (0, LANE_TRACE):
        check_occ(r.debug_occluded(seg, flags).reshape(dist.shape) != 0, occ, labels)
    assert_golden(r.render(), util.load_golden("materials_aniso")[1], "a frame after the queries")
    r.close()


@pytest.mark.parametrize("kind", ["nearest", "hits", "sweep"])
def test_walk_queries_on_one_compute_unit(api, monkeypatch, kind):
    """Their grid is cut from the spill regions, which shrank with the grids: more tiles than workgroups, against the host twin."""
    import test_gpu_query_tiles as T
    sc, rows, labels, want = T.row_set(kind, "materials_aniso")
    r = renderer(api, monkeypatch, sc)
    blocks = int(r.debug_grids()[SPILL]) // T.TILE
    assert blocks >= 1
    reps = (4 * blocks * T.TILE + len(rows) - 1) // len(rows)
    tiled = lambda a: np.concatenate([a] * reps) if isinstance(a, np.ndarray) and len(a) == len(rows) else a
    rows_t = T.dev(np.ascontiguousarray(np.concatenate([rows] * reps)))
    want_t = {k: ({j: tiled(b) for j, b in a.items()} if isinstance(a, dict) else tiled(a)) for k, a in want.items()}
    assert len(rows_t) >= 4 * blocks * T.TILE
    print(f"walk query {kind}: {len(rows_t)} rows, {(len(rows_t) + T.TILE - 1) // T.TILE} tiles over at most {blocks} workgroups")
    for sort in (False, True):
        T.compare(kind, T.run(r, kind, rows_t, sort), want_t, np.concatenate([labels] * reps), f"{kind} sort {sort}")
    r.close()


# ---- 7. contexts in flight, the group path ---------------------------------------------------------------------------------------------
def test_three_contexts_in_flight_each_with_its_own_small_grid(api, monkeypatch):
    """Three contexts on their own streams, sized for one, two and three compute units, on different scenes, queued without a host wait
    in between: each frame is its own scene's."""
    names = ("materials_aniso", "tori16", "monkey_small")
    scenes = [util.load_golden(n) for n in names]
    rs = [renderer(api, monkeypatch, sc, cus) for (sc, _), cus in zip(scenes, (1, 2, 3))]
    for r, (sc, _), name in zip(rs, scenes, names):
        past_first_round(r, sc.tile_count * 1024, what=f"in flight, {name}")
    for shape in ("serial", "default"):
        for rounds in range(3):
            for r in rs:
                r.render_async(**SHAPES[shape])
        for r, (sc, g), name in zip(rs, scenes, names):
            st, _ = r.stats(); rgb, packed = r.framebuffer()
            assert_golden({"rgb": rgb, "packed": packed, "stats": st}, g, f"{name} {shape}")
    assert len({g["packed"].tobytes() for _, g in scenes}) == 3
    for r in rs:
        r.close()


@pytest.mark.parametrize("world", [2, 3])
def test_group_loopback_on_one_compute_unit(api, monkeypatch, world):
    """The tile-major resolve and k_unswizzle with four workgroups: the assembled frame is the reference's."""
    sc, g = util.load_golden("monkey_small")
    r = renderer(api, monkeypatch, sc)
    past_first_round(r, (sc.tile_count // world) * 1024, what=f"loopback of {world}")
    for frame in range(2):
        r.group_loopback(world)
        _, packed = r.framebuffer()
        assert np.array_equal(packed, np.asarray(g["packed"]).reshape(packed.shape)), frame
    r.close()


# ---- 8. the knob itself -------------------------------------------------------------------------------------------------------------------
def test_knob_values(api, monkeypatch, capfd):
    import torch
    sc, g = util.load_golden("cube")
    device_cus = torch.cuda.get_device_properties(0).multi_processor_count
    default = [int(v) for v in renderer(api, monkeypatch, sc, None).debug_grids()]
    assert default[CUS] == device_cus
    for bad in ("0", "-3", "banana", "2.5", str(2 ** 40)):
        capfd.readouterr()
        monkeypatch.setenv("RTX_GRID_CUS", bad)
        r = api.Renderer(sc)
        assert f"RTX_GRID_CUS={bad} ignored" in capfd.readouterr().err
        assert [int(v) for v in r.debug_grids()] == default, bad
    capfd.readouterr()
    for above in (device_cus + 1, 1 << 20):                              # more than the device has: the device's count
        monkeypatch.setenv("RTX_GRID_CUS", str(above))
        assert [int(v) for v in api.Renderer(sc).debug_grids()] == default, above
    monkeypatch.setenv("RTX_GRID_CUS", str(device_cus))
    assert [int(v) for v in api.Renderer(sc).debug_grids()] == default
    assert "RTX_GRID_CUS" not in capfd.readouterr().err
    # every grid follows the count: one compute unit's grids, times the count, rounded as the packet grids are
    one = [int(v) for v in renderer(api, monkeypatch, sc, 1).debug_grids()]
    assert one[CUS] == 1 and all(1 <= a <= b for a, b in zip(one, default)) and one[SPILL] < default[SPILL]
    for k in (TRACE_CLOSEST, TRACE_ANY, TRACE_COUNT, ITEMS):
        assert one[k] * device_cus == default[k], (k, one, default)
    for k in (PK_CLOSEST, PK_ANY):
        assert one[k] % 8 == 0 and default[k] % 8 == 0 and (one[k] - 8) * device_cus < default[k] <= one[k] * device_cus + 7, (k, one, default)
    lib = api.load_library()
    out = np.zeros(8, np.int32)
    assert lib.rtx_debug_grids(None, out.ctypes.data) == 1 and lib.rtx_debug_grids(renderer(api, monkeypatch, sc).ctx, None) == 1
