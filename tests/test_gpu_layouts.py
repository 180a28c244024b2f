"""The node layouts the production kernels walk — the packet layout (pk_nodes, pk_tlas_nodes), the shadow-ray and closest-hit 4-wide records
(pk4_nodes, pk4c_nodes) and the three plane lists — read back with rtx_debug_read_layouts after rtx_refit_blas, rtx_build_blas and
rtx_update_instances wrote them, and compared with tests/layoutset.py: a numpy restatement of the record formats as functions of the lane
layout read back in the same state (rtx_read_blas / rtx_read_frame_state).  All comparisons are bit for bit; every input is legal and finite.

  baseline   plainly uploaded meshes and an uploaded TLAS: the layouts convert_nodes_pk, build_nodes_pk4 and build_nodes_pk4c made on the
             host satisfy the restatement, which pins it before it is used as a reference; meshes without a wide layout report none;
  refit      after bind, after a refit and after a second one, with and without the 4-wide layouts;
  build      after alloc, after a build, a second build and build -> refit, at the triangle counts where the tree or the launches change
             shape (the nodes equal the host twin's, as in tests/test_gpu_blas_build.py);
  update     on both paths at the instance counts where the kernels change shape (the state equals host_state, as in
             tests/test_gpu_update_instances.py), holes and index 1 zero;
  frames     one 64 x 64 frame per builder at the new sizes equals a second context given the read-back state by the plain upload path.
"""
import copy

import numpy as np
import pytest

import layoutset as ls
import util
from test_tlas_balanced_cpu import poses
from test_blas_refit_cpu import deform
from test_blas_build_cpu import refit_of_twin, soup
from test_gpu_blas_build import _meshes, base_scene, build_on_device, mesh, small, twin_of
from test_gpu_blas_refit import mesh_case
from test_gpu_rays import chain_blas_scene
from test_gpu_update_instances import assert_same_frame, assert_state, host_state, many_scene, with_state

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def dev(a, dtype=f32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def single_leaf_scene(k):
    """monkey_small with a mesh whose BVH is one leaf of k triangles (tests/test_gpu_units.py test_single_leaf_mesh)."""
    sc, _ = util.load_golden("monkey_small")
    sc = copy.deepcopy(sc)
    b = sc.blas[0]
    hot = b.tri_hot[:k].copy(); cold = b.tri_cold[:k].copy()
    pts = np.concatenate([hot["position_0"], hot["position_0"] + hot["position_edge_1"], hot["position_0"] + hot["position_edge_2"]]).astype(f32)
    nodes = np.zeros(1, util.sio.BVH_NODE)
    nodes["aabb_min"][0] = pts.min(axis=0); nodes["aabb_max"][0] = pts.max(axis=0)
    nodes["left_or_first"][0] = 0; nodes["count"][0] = k
    b.nodes = nodes; b.tri_hot = hot; b.tri_cold = cold
    return sc


def refit_mesh(name):
    """-> (scene around the mesh, slot vertices, vertices)"""
    if name == "torus_twin":                    # the balanced twin tree of the Torus under tori16 at 64 x 64
        _, sv, _, pos, _ = twin_of("torus")
        return base_scene(), sv, pos
    sc, sv, verts, _ = mesh_case(name)          # Monkey through the reference's SBVH builder: duplicated references
    return sc, sv, verts


def upload_time_planes(nodes, axis):
    """The list of a mesh that was never bound: the distinct non-NaN box coordinates, ascending (stage_blas)."""
    v = np.concatenate([nodes["aabb_min"][:, axis], nodes["aabb_max"][:, axis]]).astype(f32)
    return np.unique(v[~np.isnan(v)])


# ---- baseline: the restatement against the host conversion -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["torus_twin", "monkey_sbvh", "chain", "leaf2", "leaf40", "leaf300"])
def test_uploaded_layouts_satisfy_the_restatement(api, name):
    if name == "chain":
        sc = chain_blas_scene()
    elif name.startswith("leaf"):
        sc = single_leaf_scene(int(name[4:]))
    else:
        sc = refit_mesh(name)[0]
    r = api.Renderer(sc)
    nodes = r.read_blas(0).nodes
    assert nodes.tobytes() == np.ascontiguousarray(sc.blas[0].nodes).tobytes()
    lay = r.debug_read_layouts(0)
    assert (lay["pk4"] is not None) == (r.debug_blas_wide(0) >= 0) and (lay["pk4c"] is not None) == (r.debug_blas_wide_closest(0) >= 0)
    if name in ("torus_twin", "chain", "leaf2"):
        assert lay["pk4"] is not None and lay["pk4c"] is not None, "meant to take both 4-wide walks"
    if name == "leaf40":
        assert lay["pk4"] is not None and lay["pk4c"] is None, "a leaf of 16+ triangles keeps the binary closest-hit walk"
    if name == "leaf300":
        assert lay["pk4"] is None and lay["pk4c"] is None, "a leaf of 256+ triangles keeps both binary walks"
    if name == "monkey_sbvh":
        assert not ls.reachable(nodes).all(), "the reference's arrays leave index 1 unused"
    assert np.array_equal(lay["pk"], ls.pk(nodes)), "convert_nodes_pk converts every slot"
    ls.check_blas(nodes, lay, pk_before=ls.pk(nodes), bound=False)
    for a in range(3):
        assert np.array_equal(lay["planes"][a].view(f32), upload_time_planes(nodes, a)), a


def test_uploaded_tlas_equals_the_restatement(api):
    sc, _ = util.load_golden("tori16")
    r = api.Renderer(sc)
    _, nodes, _ = r.read_frame_state()
    assert nodes.tobytes() == np.ascontiguousarray(sc.tlas_nodes).tobytes() and len(nodes) > 2
    got = r.debug_read_layouts(-1)["pk"]
    assert np.array_equal(got, ls.pk(nodes))
    ls.check_pk(nodes, got, ls.pk(nodes))


# ---- after bind, after refit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("name", ["torus_twin", "monkey_sbvh"])
def test_layouts_after_bind_and_refit(api, name, wide, monkeypatch):
    from pyrtx import host
    if not wide:
        monkeypatch.setenv("RTX_PK_WIDE", "0"); monkeypatch.setenv("RTX_PK_WIDE_CLOSEST", "0")
    sc, sv, verts = refit_mesh(name)
    r = api.Renderer(sc)
    up = r.debug_read_layouts(0)
    if not wide:
        assert up["pk4"] is None and up["pk4c"] is None
    elif name == "torus_twin":
        assert up["pk4"] is not None and up["pk4c"] is not None
    r.bind_blas_vertices(0, sv, len(verts))
    blas = r.read_blas(0)
    assert blas.nodes.tobytes() == np.ascontiguousarray(sc.blas[0].nodes).tobytes()
    bound = r.debug_read_layouts(0)
    for k in ("pk", "pk4", "pk4c"):             # the bind rewrites every box with the value it has
        assert (bound[k] is None) == (up[k] is None) and (up[k] is None or np.array_equal(bound[k], up[k])), k
    ls.check_blas(blas.nodes, bound, pk_before=up["pk"], pk4_before=up["pk4"])
    want = sc.blas[0]
    for step, moved in enumerate((deform(verts, "wave", seed=21), deform(verts, "twist", seed=5))):
        v = dev(moved)
        r.refit_blas(0, v)
        want = host.blas_refit(want, sv, moved)
        nodes = r.read_blas(0).nodes
        assert nodes.tobytes() == want.nodes.tobytes(), step
        lay = r.debug_read_layouts(0)
        assert (lay["pk4"] is None) == (up["pk4"] is None) and (lay["pk4c"] is None) == (up["pk4c"] is None), step
        ls.check_blas(nodes, lay, pk_before=bound["pk"], pk4_before=bound["pk4"])
        assert not np.array_equal(lay["pk"], bound["pk"]), "the deformation must show"


# ---- after alloc, after build ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup1", "soup4", "soup5", "soup8", "soup9", "soup4096", "soup4097", "soup20000", "identical", "padded"])
def test_layouts_after_alloc_and_build(api, name):
    from pyrtx import host
    pos, idx, nrm, uv, mid, bad = mesh(name)
    T = len(idx)
    r = api.Renderer(base_scene())
    r.alloc_blas(0, T, len(pos), mid)
    empty = r.read_blas(0).nodes
    alloc = r.debug_read_layouts(0)
    assert alloc["pk4"] is not None and alloc["pk4c"] is not None, "the balanced tree takes both 4-wide walks"
    assert len(empty) == host.blas_balanced_node_count(T)
    ls.check_blas(empty, alloc)
    if T <= 4:
        assert not alloc["pk4"].any() and not alloc["pk4c"].any(), "the root is a leaf: no records"
    for variant in (0, 1):                      # a build, and a second one over it with other vertices
        build_on_device(r, name, True, variant, alloc=False)
        want, sv, _, moved, moved_n = twin_of(name, True, variant)
        nodes = r.read_blas(0).nodes
        assert nodes.tobytes() == want.nodes.tobytes(), variant
        lay = r.debug_read_layouts(0)
        ls.check_blas(nodes, lay, pk4_before=alloc["pk4"])
        assert np.array_equal(lay["pk4c"][:, 6], alloc["pk4c"][:, 6]), "the `first` words of the closest-hit records are the alloc's"
    if name == "padded":
        assert len(bad) and (sv < 0).any()
    again = deform(moved, "wave", seed=21) if len(moved) > 12 else np.ascontiguousarray(moved * f32(0.75) + f32(0.125))
    v = dev(again)
    r.refit_blas(0, v)                          # build -> refit: the axis fields of the last build stay
    ref = refit_of_twin(want, sv, again)
    nodes = r.read_blas(0).nodes
    assert nodes.tobytes() == ref.nodes.tobytes()
    after = r.debug_read_layouts(0)
    ls.check_blas(nodes, after, pk4_before=lay["pk4"])
    assert np.array_equal(after["pk4c"][:, 6:], lay["pk4c"][:, 6:]), "a refit keeps first and meta"


# ---- after update ----------------------------------------------------------------------------------------------------------------------
_many = {}


def update_case(n):
    """-> (scene of n instances, two sets of poses with their host states)"""
    if n not in _many:
        if n == "same33":                       # every Morton cell is 0 / 0: the index alone decides the order
            sc, pos, rot = many_scene(33, 33)
            sets = [(np.ascontiguousarray(np.broadcast_to(p, pos.shape), f32), rot) for p in (f32([1.5, 4.0, 12.0]), f32([-2.0, 3.0, 15.0]))]
        else:
            sc, pos, rot = many_scene(n, 100 + n)
            sets = [((pos * f32(1.01)).astype(f32), rot), ((pos[::-1] * f32(0.97)).astype(f32), rot)]
        _many[n] = (sc, [(p, q, host_state(sc, p, q)) for p, q in sets])
    return _many[n]


@pytest.mark.parametrize("path", ["one_workgroup", "multi_launch"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 64, 65, 1023, 1024, 1025, 2048, 2049, "same33"])
def test_tlas_packet_layout_after_update(api, n, path, monkeypatch):
    if path == "multi_launch":
        monkeypatch.setenv("RTX_UPDATE_SMALL_MAX", "0")
    sc, sets = update_case(n)
    r = api.Renderer(sc)
    for step, (pos, rot, want) in enumerate(sets):
        p, q = dev(pos), dev(rot)
        r.update_instances(p, q)
        state = r.read_frame_state()
        assert_state(state, want, f"n = {n}, {path}, step {step}")
        nodes = state[1]
        reach = ls.reachable(nodes)
        assert not nodes[~reach].tobytes().strip(b"\0") and not reach[1], "holes and index 1 are zero bytes"
        ls.check_pk(nodes, r.debug_read_layouts(-1)["pk"])
        if n == "same33":
            assert np.array_equal(state[2], np.arange(33)), "ties are broken by the instance index"


# ---- one rendered frame per builder at the new sizes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [{}, {"serial": True}], ids=["default", "serial"])
def test_frame_of_1025_updated_instances_equals_the_set_frame_path(api, mode):
    sc, sets = update_case(1025)
    sc = small(sc)
    pos, rot, want = sets[0]
    r = api.Renderer(sc)
    p, q = dev(pos), dev(rot)
    r.update_instances(p, q)
    out = r.render(**mode)
    state = r.read_frame_state()
    assert_state(state, want)
    ls.check_pk(state[1], r.debug_read_layouts(-1)["pk"])
    assert_same_frame(out, api.Renderer(with_state(sc, state)).render(**mode), "second context")
    assert out["stats"]["primary"] == 64 * 64 and len(np.unique(out["packed"])) > 16, "the instances are meant to show"


def big9():
    """soup(9) with every triangle enlarged about its centre and the centres drawn together: nine triangles a 64 x 64 frame shows.
    Registered with test_gpu_blas_build's meshes, so that twin_of and build_on_device know it by name."""
    if "big9" not in _meshes:
        pos, idx, nrm, uv, mid = soup(9, 7)
        tri = pos.reshape(9, 3, 3).astype(np.float64)
        c = tri.mean(1, keepdims=True)
        _meshes["big9"] = (np.ascontiguousarray((0.4 * c + 8.0 * (tri - c)).reshape(-1, 3), f32), idx, nrm, uv, mid, np.zeros(0, np.int64))
    return _meshes["big9"]


@pytest.mark.parametrize("mode", [{}, {"serial": True}], ids=["default", "serial"])
def test_frame_of_the_nine_triangle_build_equals_the_upload_path(api, mode):
    sc = base_scene()
    pos, idx, nrm, uv, mid, _ = big9()
    r = api.Renderer(sc)
    r.alloc_blas(0, len(idx), len(pos), mid)
    pp, qq = poses("tori16", 1)
    p, q = dev(pp), dev(qq)
    r.update_instances(p, q)
    empty = r.render(**mode)
    build_on_device(r, "big9", alloc=False)
    r.update_instances(p, q)                    # the world boxes and the TLAS over the new root box
    out = r.render(**mode)
    got = r.read_blas(0)
    assert got.nodes.tobytes() == twin_of("big9")[0].nodes.tobytes()
    ls.check_blas(got.nodes, r.debug_read_layouts(0))
    second = copy.copy(sc); second.blas = [got]
    second = with_state(second, r.read_frame_state())
    r2 = api.Renderer(second)
    assert r2.debug_blas_wide(0) >= 0 and r2.debug_blas_wide_closest(0) >= 0
    assert_same_frame(out, r2.render(**mode), "second context")
    assert not np.array_equal(out["packed"], empty["packed"]), "the nine triangles are meant to show"
