"""The packet kernels' direct entry of a lone instance (csrc/rtx_plan.h plan_lone_facts, csrc/rtx_packet.h pk_enter; RTX_PK_LONE_ENTRY).

A frame whose TLAS is one leaf holding one instance is entered straight from the packet set-up, and where the instance's world_inv is of the
copy class (1.0f on the diagonal, +-0 elsewhere) a packet none of whose valid lanes has a zero component keeps the world-space ray.  Both are
decided per frame on the host and per packet by a ballot, so the shapes here are the smallest at which that can go wrong: one small mesh,
frames and ray sets of two 8 x 8 packets (16 x 8 pixels: slot l of a tile is pixel l & 63 of block l >> 6), one packet all ordinary, one mixed.
Everything is compared bit for bit (NaN == NaN), ray counts included, with the oracle, and with RTX_RENDER_LANE_TRACE — the per-lane kernels
have no such path — and the knob's two values with each other.  What the host decided is pinned on the CPU (csrc/lone_check.cpp,
tests/test_lone_entry_cpu.py); here `facts` restates it in numpy so that every case asserts which path it is about."""
import copy

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W, H = 16, 8                                     # two packets side by side
NEG0 = f32(-0.0)
_ORACLE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def shrunk(name, w=W, h=H, bounces=None):
    """The golden scene at w x h: the camera's pixel axes stretched so that the frame keeps the golden's field of view."""
    sc = copy.deepcopy(util.load_golden(name)[0])
    w0, h0 = sc.width, sc.height
    sc.config["width"] = w; sc.config["height"] = h
    cam = sc.camera.copy()
    cam["rotated_x_axis"] = (cam["rotated_x_axis"].astype(f64) * (w0 / w)).astype(f32)
    cam["rotated_y_axis"] = (cam["rotated_y_axis"].astype(f64) * (h0 / h)).astype(f32)
    sc.camera = cam
    if bounces is not None:
        sc.config["bounces"] = bounces
    return sc


def aimed(sc, position, target, zoom=1.0):
    """sc seen from `position` towards `target`: a camera in general position (no axis of it along a world axis), `zoom` frame widths from its image plane."""
    sc = copy.deepcopy(sc)
    w, h = sc.width, sc.height
    p, t = np.asarray(position, f64), np.asarray(target, f64)
    fwd = (t - p) / np.linalg.norm(t - p)
    right = np.cross([0.0, 1.0, 0.0], fwd); right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    cam = sc.camera.copy()
    cam["position"] = p.astype(f32)
    cam["rotated_x_axis"] = right.astype(f32); cam["rotated_y_axis"] = (-up).astype(f32)
    cam["rotated_top_left_corner"] = (fwd * (zoom * w) - right * (w / 2) + up * (h / 2)).astype(f32)
    sc.camera = cam
    return sc


def cube(w=W, h=H):
    """The cube golden (one instance at the origin, identity matrices, a point light) with two bounces, every material reflecting and
    transmitting, seen from close by: closest-hit packets of levels 0 .. 2 (the refracted rays hit the cube from inside) and shadow-ray
    packets of every level."""
    sc = aimed(shrunk("cube", w, h, bounces=2), (2.1, 1.3, -2.6), (0.1, 0.05, 0.0))
    mats = sc.materials.copy()
    mats["reflection"] = 0.5; mats["transmittance"] = 0.5
    sc.materials = mats
    return sc


def facts(sc):
    """plan_lone_facts (csrc/rtx_plan.h) in numpy -> (lone, copy_class)."""
    lone = (len(sc.instances) == 1 and len(sc.tlas_nodes) >= 1 and len(sc.tlas_indices) >= 1 and int(sc.tlas_nodes[0]["count"]) == 1
            and int(sc.tlas_nodes[0]["left_or_first"]) == 0 and int(sc.tlas_indices[0]) == 0)
    if not lone:
        return False, False
    bits = np.ascontiguousarray(sc.instances["world_inv"][0], f32).view(np.uint32)[:12]
    diagonal = np.isin(np.arange(12), (0, 5, 10))
    return True, bool(np.all(bits[diagonal] == 0x3f800000) and np.all((bits[~diagonal] & 0x7fffffff) == 0))


def with_world_inv(sc, cells):
    """A copy of sc whose one instance has world_inv cells {index: value} written over what it had."""
    sc = copy.deepcopy(sc)
    inst = sc.instances.copy()
    wi = inst["world_inv"][0].copy()
    for k, v in cells.items():
        wi[k] = v
    inst["world_inv"][0] = wi
    sc.instances = inst
    return sc


def posed(sc, positions, rotations):
    """sc with its instances at the poses, the matrices and the balanced TLAS Scene::update makes of them (what rtx_update_instances builds)."""
    from pyrtx import host
    from test_gpu_update_instances import with_state
    return with_state(copy.deepcopy(sc), host.scene_update_balanced(sc, positions, rotations))


def oracle_frame(key, sc):
    if key not in _ORACLE:
        import orc
        _ORACLE[key] = orc.OracleScene(sc).render(threads=8)
    return _ORACLE[key]


def assert_frame(out, ref, what):
    assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])
    assert util.bit_exact(out["rgb"], ref["rgb"]), f"{what}: rgb differs"
    assert np.array_equal(out["packed"], ref["packed"]), what


def renderer(api, monkeypatch, sc, **knobs):
    """A fresh context: the knobs are read once, in rtx_create."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    r = api.Renderer(sc)
    for k in knobs:
        monkeypatch.delenv(k)
    return r


def frames_on_both_paths(api, monkeypatch, sc, ref, what):
    """The frame by the packet kernels with the direct entry and without it, and by the per-lane kernels: each equals `ref`."""
    for lone_entry in (1, 0):
        r = renderer(api, monkeypatch, sc, RTX_PK_LONE_ENTRY=lone_entry)
        assert_frame(r.render(), ref, f"{what}, RTX_PK_LONE_ENTRY={lone_entry}")
        assert_frame(r.render(serial=True), ref, f"{what}, RTX_PK_LONE_ENTRY={lone_entry}, serial")
        if lone_entry:
            assert_frame(r.render(lane_trace=True), ref, f"{what}, lane trace")
        r.close()


# ---- matrix variants, written directly into the instance record ------------------------------------------------------------------------------------
OFF_DIAGONAL = (1, 2, 3, 4, 6, 7, 8, 9, 11)
MATRICES = {
    "all_plus_zero": ({k: f32(0.0) for k in OFF_DIAGONAL}, True),
    "minus_zero_cells": ({1: NEG0, 6: NEG0, 8: NEG0, 3: NEG0, 7: NEG0, 11: NEG0}, True),
    "all_minus_zero": ({k: NEG0 for k in OFF_DIAGONAL}, True),
    "diagonal_one_ulp_up": ({5: np.nextafter(f32(1.0), f32(2.0))}, False),
    "off_diagonal_1e-45": ({2: np.uint32(1).view(f32)}, False),
}


@pytest.mark.parametrize("variant", list(MATRICES))
def test_matrix_variants_equal_the_oracle(api, monkeypatch, variant):
    """The oracle multiplies by the world_inv it is handed, whatever `world` says: cells of the copy class skip the product in the packet
    kernels, a diagonal of 1 + 2^-23 or a 1e-45 cell must take it."""
    cells, want_copy = MATRICES[variant]
    sc = with_world_inv(cube(), cells)
    assert facts(sc) == (True, want_copy)
    frames_on_both_paths(api, monkeypatch, sc, oracle_frame(("matrix", variant), sc), variant)


# ---- zero components: caller-supplied rays ---------------------------------------------------------------------------------------------------------
def zero_component_rays(api, sc):
    """(H, W, 18) rays of the scene's camera.  The left packet is left as it is (no zero component: asserted); in the right packet lanes get
    d.x = +0, d.x = -0, d.y = -0 with the other two negative, and origins with a +0 / -0 component; the rest stay ordinary."""
    rays = api.pinhole_rays(sc.camera[0], W, H).copy()
    assert np.all(rays[:, :8, :6] != 0), "the ordinary packet has no zero component"
    right = rays[:, 8:, :]
    right[0, 0, 3] = f32(0.0)
    right[0, 1, 3] = NEG0
    right[1, 0, 3:6] = (-0.6, NEG0, -0.8)
    right[1, 1, 3:6] = (NEG0, -0.6, -0.8)
    right[2, 0, 0] = f32(0.0)
    right[2, 1, 1] = NEG0
    right[3, 0, 2] = NEG0; right[3, 0, 3:6] = (-0.3, -0.4, f32(0.0))
    right[4, 2, 0:3] = (NEG0, f32(0.0), right[4, 2, 2])
    assert np.all(rays[:, 8:, :6][5:] != 0), "and ordinary lanes remain in the mixed packet"
    return rays


@pytest.mark.parametrize("variant", ["all_plus_zero", "all_minus_zero", "minus_zero_cells"])
def test_zero_components_take_the_arithmetic(api, monkeypatch, variant):
    """A zero component can leave the product with the other sign, and 1 / +-0 is a sign the slab test reads: the packet that holds one takes
    the arithmetic, the packet beside it does not.  render_rays, then the same rays through the ray queries (level-1 closest-hit packets, the
    explicit shadow rays), against the oracle and the per-lane kernels."""
    import orc
    from test_gpu_query import check_channels, dev, expected, host as to_host, segments_of
    from test_gpu_rays import check_occ
    sc = with_world_inv(cube(), MATRICES[variant][0])
    assert facts(sc) == (True, True)
    rays = zero_component_rays(api, sc)
    o = orc.OracleScene(sc)
    ref = o.shade_rays(rays)
    assert ref["stats"]["primary"] == W * H and ref["stats"]["shadow"] > 0 and ref["stats"]["reflection"] + ref["stats"]["refraction"] > 0
    rays6 = np.ascontiguousarray(rays.reshape(-1, 18)[:, :6])
    want = expected(o, rays6)
    hits, _ = o.trace_closest(rays.reshape(-1, 18))
    dist = np.where(hits[:, 0] > 0, hits[:, 1] * f32(1.5), f32(50.0)).astype(f32)[:, None]      # beyond the first hit: occluded where there is one
    occ = o.trace_any(rays.reshape(-1, 18), dist)
    assert occ.any() and not occ.all()
    labels = np.where(np.arange(W * H).reshape(H, W) % W < 8, "ordinary", "mixed").reshape(-1)
    for lone_entry in (1, 0):
        r = renderer(api, monkeypatch, sc, RTX_PK_LONE_ENTRY=lone_entry)
        r.set_rays(rays)
        for flags in ({}, {"serial": True}, {"lane_trace": True}):
            out = r.render_rays(**flags)
            what = f"{variant}, RTX_PK_LONE_ENTRY={lone_entry}, {flags}"
            assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])
            assert util.bit_exact(out["rgb"][0], ref["rgb"]) and np.array_equal(out["packed"][0], ref["packed"]), what
        for kw in ({}, {"lane_trace": True}):
            check_channels(r.query_closest(dev(rays6), tuple(api.QUERY_CHANNELS), **kw), want, labels, f"{variant} {lone_entry} {kw}")
            got = to_host(r.query_occluded(dev(segments_of(rays6, dist)), **kw))
            check_occ(got.reshape(dist.shape) != 0, occ, labels)
        r.close()


# ---- a lone instance that is rotated and translated: the direct entry without the transform skip --------------------------------------------------
def test_a_rotated_and_translated_lone_instance(api, monkeypatch):
    from pyrtx import host
    sc = posed(cube(), [[0.4, -0.25, 0.3]], [host.axis_angle((0.3, 1.0, -0.2), 0.6)])
    assert facts(sc) == (True, False)
    frames_on_both_paths(api, monkeypatch, sc, oracle_frame("turned", sc), "rotated and translated")


def test_a_lone_instance_posed_at_the_origin_by_the_host(api, monkeypatch):
    """Scene::update's own identity pose, through the cofactor inverse: whatever zeros it leaves, the record is of the copy class."""
    sc = posed(cube(), [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 1.0]])
    assert facts(sc) == (True, True)
    frames_on_both_paths(api, monkeypatch, sc, oracle_frame("host identity", sc), "posed at the origin")


# ---- scenes that are not lone ------------------------------------------------------------------------------------------------------------------------
def two_instances():
    sc = cube()
    inst = np.concatenate([sc.instances, sc.instances])
    sc.instances = inst
    return posed(sc, [[0.0, 0.0, 0.0], [1.5, 0.5, 1.0]], [[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0]])


def two_in_one_leaf():
    """two instances under a TLAS whose root is a leaf of two: the iterator entry with something left in it"""
    sc = two_instances()
    lo = np.minimum(sc.tlas_nodes[2]["aabb_min"], sc.tlas_nodes[3]["aabb_min"]); hi = np.maximum(sc.tlas_nodes[2]["aabb_max"], sc.tlas_nodes[3]["aabb_max"])
    nodes = sc.tlas_nodes[:2].copy()
    nodes[0]["aabb_min"] = lo; nodes[0]["aabb_max"] = hi; nodes[0]["left_or_first"] = 0; nodes[0]["count"] = 2
    sc.tlas_nodes = nodes; sc.tlas_indices = np.array([1, 0], np.int32)
    return sc


def no_instance():
    from pyrtx import scene_io as sio
    sc = shrunk("materials_aniso")
    sc.instances = np.zeros(0, sio.INSTANCE); sc.tlas_nodes = np.zeros(0, sio.BVH_NODE); sc.tlas_indices = np.zeros(0, np.int32)
    return sc


NOT_LONE = {"two_instances": two_instances, "two_in_one_leaf": two_in_one_leaf, "spheres_and_planes_first": lambda: shrunk("materials_aniso"),
            "no_instance": no_instance, "coincident": lambda: shrunk("coincident")}


@pytest.mark.parametrize("name", list(NOT_LONE))
def test_scenes_that_are_not_lone_keep_the_iterator_path(api, monkeypatch, name):
    sc = NOT_LONE[name]()
    assert facts(sc) == (False, False)
    if name == "two_instances":
        assert int(sc.tlas_nodes[0]["count"]) & 0x3fffffff == 0 and len(sc.tlas_nodes) == 4      # an inner root over two leaves
    frames_on_both_paths(api, monkeypatch, sc, oracle_frame(("not lone", name), sc), name)


def test_one_instance_beside_spheres_and_planes(api, monkeypatch):
    """lone, with the spheres and the plane of the materials golden tested before the TLAS: lanes they occlude or hit nearer enter with the rest"""
    sc = shrunk("materials_aniso")
    keep = 0
    one = copy.deepcopy(sc)
    one.instances = sc.instances[keep:keep + 1].copy()
    pos = one.instances["world"][0].reshape(4, 4)[:3, 3]
    one = posed(one, [pos], [[0.0, 0.0, 0.0, 1.0]])
    assert facts(one)[0] and len(one.spheres) == 2 and len(one.planes) == 1
    frames_on_both_paths(api, monkeypatch, one, oracle_frame("one beside primitives", one), "one instance beside spheres and a plane")


# ---- the knob crossed with the launch shapes ------------------------------------------------------------------------------------------------------
SHAPES = {"default": ({}, {}), "serial": ({}, {"serial": True}), "no_split": ({"RTX_PK_SPLIT": 0}, {}), "fused": ({"RTX_FUSE_SHADE": 1}, {}),
          "fused_cull": ({"RTX_FUSE_SHADE": 1}, {"cull_dead_shadow_rays": True}), "packet_closest": ({}, {"packet_closest": True}),
          "packet_stats": ({}, {"packet_stats": True}), "graph": ({"RTX_GRAPH": 1}, {})}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("lone_entry", [0, 1])
def test_knob_matrix_frames_and_stats(api, monkeypatch, lone_entry, shape):
    """24 x 12: six packets, the lower three half empty.  Each context renders three times (a graph is captured and replayed)."""
    sc = cube(24, 12)
    assert facts(sc) == (True, True)
    ref = oracle_frame("knob matrix", sc)
    assert ref["stats"]["shadow"] > 0 and ref["stats"]["reflection"] + ref["stats"]["refraction"] > 0
    knobs, flags = SHAPES[shape]
    r = renderer(api, monkeypatch, sc, RTX_PK_LONE_ENTRY=lone_entry, **knobs)
    for k in range(3):
        assert_frame(r.render(**flags), ref, f"{shape}, RTX_PK_LONE_ENTRY={lone_entry}, frame {k}")
    r.close()


@pytest.mark.parametrize("lone_entry", [0, 1])
def test_knob_with_aovs_and_a_batch_of_two_views(api, monkeypatch, lone_entry):
    from test_gpu_views import with_camera
    sc = cube(24, 12)
    ref = oracle_frame("knob matrix", sc)
    r = renderer(api, monkeypatch, sc, RTX_PK_LONE_ENTRY=lone_entry)
    out = r.render_aovs(("depth", "object_id"))
    assert_frame(out, ref, "the AOV call's colours")
    lane = r.render_aovs(("depth", "object_id"), lane_trace=True)
    assert util.bit_exact(out["depth"], lane["depth"]) and np.array_equal(out["object_id"], lane["object_id"]) and np.isfinite(out["depth"]).any()
    moved = sc.camera.copy(); moved["position"] = moved["position"] + f32([0.25, 0.1, -0.2])
    cams = np.concatenate([sc.camera, moved])
    r.set_views(cams)
    views = r.render_views()
    for k in range(2):
        one = oracle_frame(("knob matrix view", k), with_camera(sc, cams[k]))
        assert util.bit_exact(views["rgb"][k], one["rgb"]) and np.array_equal(views["packed"][k], one["packed"]), k
    assert views["stats"] == {n: ref["stats"][n] + oracle_frame(("knob matrix view", 1), with_camera(sc, cams[1]))["stats"][n] for n in ref["stats"]}
    r.close()


# ---- a context over time -----------------------------------------------------------------------------------------------------------------------------
def test_a_context_over_time(api):
    """copy class -> the instance moved by a frame state (both facts drop) -> rtx_update_instances from device memory back to the origin (facts
    cleared: the host has not seen those matrices, though they are of the copy class) -> the first state again.  Twice round."""
    from pyrtx import host
    from test_gpu_query import dev
    from test_gpu_update_instances import with_state
    sc = cube()
    moved = posed(sc, [[0.3, 0.2, -0.4]], [host.axis_angle((0.0, 1.0, 0.1), 0.4)])
    assert facts(sc) == (True, True) and facts(moved) == (True, False)
    origin = posed(sc, [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 1.0]])
    p_t, q_t = dev(np.zeros((1, 3), f32)), dev(np.array([[0.0, 0.0, 0.0, 1.0]], f32))
    r = api.Renderer(sc)
    for turn in range(2):
        assert_frame(r.render(), oracle_frame("time first", sc), f"first state, turn {turn}")
        r.set_frame(moved)
        assert_frame(r.render(), oracle_frame("time moved", moved), f"moved, turn {turn}")
        r.update_instances(p_t, q_t)
        state = r.read_frame_state()
        assert state[0].tobytes() == origin.instances.tobytes() and facts(with_state(sc, state)) == (True, True)
        assert_frame(r.render(), oracle_frame("time origin", origin), f"after rtx_update_instances, turn {turn}")
        assert_frame(r.render(lane_trace=True), oracle_frame("time origin", origin), f"after rtx_update_instances, lane trace, turn {turn}")
        r.set_frame(sc)
    assert_frame(r.render(), oracle_frame("time first", sc), "the first state at the end")
    r.close()


# ---- the NaN rule from the new entry ------------------------------------------------------------------------------------------------------------------
def inner_plane(sc, axis):
    """A box-plane coordinate of the mesh on `axis` that is no plane of its root box (and so of no TLAS box)."""
    import affineset
    blas = sc.blas[int(sc.instances["blas_id"][0])]
    planes = affineset.node_planes(blas, axis)
    root = (f32(blas.nodes[0]["aabb_min"][axis]), f32(blas.nodes[0]["aabb_max"][axis]))
    tlas = np.concatenate([sc.tlas_nodes[:1]["aabb_min"][:, axis], sc.tlas_nodes[:1]["aabb_max"][:, axis]])
    inner = [p for p in planes if p not in root and p not in tlas]
    assert inner, "the mesh has an inner box plane on this axis"
    return f32(inner[len(inner) // 2])


def on_plane_camera(sc, x):
    """An axis-aligned camera looking down +z from x = `x`: the pixel column W / 2 has d.x == 0 exactly, so its rays run inside the plane
    x = `x`; no other component of any ray is zero (the rows are half a pixel off the axis)."""
    sc = copy.deepcopy(sc)
    cam = sc.camera.copy()
    cam["position"] = (x, 0.25, -4.0)
    cam["rotated_x_axis"] = (1.0, 0.0, 0.0); cam["rotated_y_axis"] = (0.0, -1.0, 0.0)
    cam["rotated_top_left_corner"] = (-W / 2, H / 2 + 0.5, 1.5 * W)
    sc.camera = cam
    return sc


@pytest.mark.parametrize("variant", ["all_plus_zero", "all_minus_zero"])
@pytest.mark.parametrize("where", ["mesh_plane", "root_plane"])
def test_the_nan_rule_from_the_direct_entry(api, monkeypatch, where, variant):
    """A camera on a box plane with a zero direction component: 0 * inf in the slab test, the one place where the sign of a zero decides
    (a < b ? a : b keeps b for a NaN), and so the place where a world_inv of -0 cells could show.  mesh_plane: a plane of an inner node of the mesh
    and of no TLAS box, so the packet starts in the fast walker and the direct entry must hand it to the reference-form one; root_plane: the
    plane is the TLAS box's too, and the packet starts in the reference-form walker.  monkey_small's mesh (776 triangles: inner planes)."""
    base = with_world_inv(shrunk("monkey_small"), MATRICES[variant][0])
    blas = base.blas[0]
    x = inner_plane(base, 0) if where == "mesh_plane" else f32(blas.nodes[0]["aabb_min"][0])
    sc = on_plane_camera(base, x)
    assert facts(sc) == (True, True)
    rays = api.pinhole_rays(sc.camera[0], W, H)
    assert np.all(rays[:, W // 2, 3] == 0) and np.all(rays[..., 0] == x) and np.all(rays[:, :8, :6] != 0)      # the left packet is ordinary
    ref = oracle_frame(("nan rule", where, variant), sc)
    assert ref["stats"]["primary"] == W * H
    frames_on_both_paths(api, monkeypatch, sc, ref, f"{where} {variant}")


def test_the_nan_rule_where_the_transform_is_skipped(api, monkeypatch):
    """Direction components of 1e-45 are not zero — the packet keeps the world-space ray — but their reciprocal is infinite, and the origins
    lie on an inner box plane of the mesh: the skipped transform must still hand the packet to the reference-form walker."""
    import orc
    base = shrunk("monkey_small")
    x = inner_plane(base, 0)
    sc = on_plane_camera(base, x)
    rays = api.pinhole_rays(sc.camera[0], W, H).copy()
    tiny = np.uint32(1).view(f32)
    rays[:, W // 2, 3] = tiny                       # the column that had d.x == 0, in the right packet
    rays[:, 2, 3] = -tiny                           # and one in the left packet
    with np.errstate(over="ignore"):
        assert np.all(rays[..., :6] != 0) and np.all(np.isinf(f32(1.0) / rays[:, W // 2, 3]))
    ref = orc.OracleScene(sc).shade_rays(rays)
    for lone_entry in (1, 0):
        r = renderer(api, monkeypatch, sc, RTX_PK_LONE_ENTRY=lone_entry)
        r.set_rays(rays)
        for flags in ({}, {"lane_trace": True}):
            out = r.render_rays(**flags)
            assert out["stats"] == ref["stats"], (lone_entry, flags, out["stats"], ref["stats"])
            assert util.bit_exact(out["rgb"][0], ref["rgb"]) and np.array_equal(out["packed"][0], ref["packed"]), (lone_entry, flags)
        r.close()
