"""Replacing what a long-lived context holds: a BLAS id re-uploaded, refused, bound and refitted; the three staging rings wrapped and grown;
the context's AOV buffers grown.  One rule is checked throughout: a call that is refused changes nothing, and a call that replaces or grows
a buffer keeps what the next call is entitled to find there.

Everything is the `cube` golden scene at 64x64 on one context, compared bit for bit (float arrays as uint32) with frames of the same
context or of a fresh one given the same uploads.  No call here reaches the device with bad input: every refusal is the host's validation.
"""
import copy

import numpy as np
import pytest

import util
from test_gpu_ray_views import assert_same, camera_rays
from test_gpu_views import camera_set, with_camera

pytestmark = pytest.mark.gpu
f32 = np.float32
SIDE = 64
INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def cube_scene():
    """the golden cube scene at 64x64: the same field of view over a quarter of the pixels per axis"""
    sc = util.load_golden("cube")[0]
    k = f32(sc.width / SIDE)
    sc.config["width"] = SIDE; sc.config["height"] = SIDE
    sc.camera = sc.camera.copy()
    sc.camera["rotated_x_axis"] *= k; sc.camera["rotated_y_axis"] *= k
    return sc


def monkey_blas(sc):
    """monkey_small's BLAS with the cube's material offset: a different mesh that is legal under the cube's id"""
    mk = copy.copy(util.load_golden("monkey_small")[0].blas[0])
    mk.material_offset = sc.blas[0].material_offset
    return mk


def upload_blas(r, blas_id, b, nodes=None, cold=None):
    """rtx_upload_blas itself, returning the status"""
    nodes = np.ascontiguousarray(b.nodes if nodes is None else nodes); hot = np.ascontiguousarray(b.tri_hot)
    cold = np.ascontiguousarray(b.tri_cold if cold is None else cold)
    rc = r.lib.rtx_upload_blas(r.ctx, blas_id, nodes.ctypes.data, len(nodes), hot.ctypes.data, cold.ctypes.data, len(hot), b.material_offset)
    if rc == 0:
        r._blas_shapes[blas_id] = (len(nodes), len(hot), b.material_offset, b.source_triangle_count)
    return rc


def negative_material(b):
    cold = b.tri_cold.copy()
    cold["material_id"][len(cold) // 2] = -1
    return cold


def leaf_past_the_end(b):
    """the tree with one reachable leaf's range moved past triangle_count"""
    nodes = b.nodes.copy()
    i = 0
    while (nodes["count"][i] & 0x3fffffff) == 0:
        i = int(nodes["left_or_first"][i])
    nodes["left_or_first"][i] = len(b.tri_hot)
    return nodes


def assert_frame(out, ref, what):
    assert_same(out["rgb"], ref["rgb"], what + " rgb")
    assert_same(out["packed"], ref["packed"], what + " packed")
    assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])


def assert_blas(got, want, what):
    for part in ("nodes", "tri_hot", "tri_cold"):
        assert getattr(got, part).tobytes() == getattr(want, part).tobytes(), (what, part)


def soup_of(b):
    """Vertices whose refit reproduces b's hot triangles bit for bit: slot s has vertices 3s .. 3s+2 = p0 and, for each edge, the fp32 value v
    next to p0 + e with fl(v - p0) == e (the vertex the edge was computed from is one such value)."""
    hot = b.tri_hot
    p0 = hot["position_0"].astype(f32)
    verts = np.zeros((len(hot), 3, 3), f32)
    verts[:, 0] = p0
    for c, name in ((1, "position_edge_1"), (2, "position_edge_2")):
        e = hot[name].astype(f32)
        v = (p0 + e).astype(f32)
        for step in (0, 1, -1, 2, -2, 3, -3):
            cand = (p0 + e).astype(f32)
            for _ in range(abs(step)):
                cand = np.nextafter(cand, f32(np.inf if step > 0 else -np.inf)).astype(f32)
            fix = ((v - p0).astype(f32) != e) & ((cand - p0).astype(f32) == e)
            v = np.where(fix, cand, v)
        assert np.array_equal((v - p0).astype(f32), e), name
        verts[:, c] = v
    return np.arange(3 * len(hot), dtype=np.int32).reshape(-1, 3), verts.reshape(-1, 3)


def test_refused_reupload_changes_nothing(api):
    """rtx_upload_blas of another mesh under the cube's id, refused for a negative triangle material id and for a leaf range past
    triangle_count: RTX_ERR_INVALID_ARG, the next frame and rtx_read_blas still show the cube (the frame set earlier refers to that id)."""
    sc = cube_scene()
    r = api.Renderer(sc)
    A = r.render()
    assert len(np.unique(A["packed"])) > 1                                       # the cube is in view
    mk = monkey_blas(sc)
    for what, bad in (("negative material id", {"cold": negative_material(mk)}), ("leaf past triangle_count", {"nodes": leaf_past_the_end(mk)})):
        assert upload_blas(r, 0, mk, **bad) == INVALID, what
        assert_frame(r.render(), A, "after the upload refused for a " + what)
        assert_blas(r.read_blas(0), sc.blas[0], what)
    for what, bad in (("negative material id", {"cold": negative_material(mk)}), ("leaf past triangle_count", {"nodes": leaf_past_the_end(mk)})):
        assert upload_blas(r, 3, mk, **bad) == INVALID, what                     # an id that held nothing stays empty
        assert r.lib.rtx_read_blas(r.ctx, 3, None, None, None) == STATE, what
    assert_frame(r.render(), A, "after refused uploads under a new id")
    r.close()


def test_replacement_after_a_refused_upload(api):
    """After a refused upload the id takes the other mesh, a vertex binding with a refit, and the cube again: every frame is the frame of a
    fresh context given the same uploads, and the re-upload drops the binding."""
    import torch
    sc = cube_scene()
    r = api.Renderer(sc)
    A = r.render()
    mk = monkey_blas(sc)
    assert upload_blas(r, 0, mk, cold=negative_material(mk)) == INVALID
    assert upload_blas(r, 0, mk) == 0
    r.set_frame(sc)
    B = r.render()
    sc2 = copy.copy(sc); sc2.blas = [mk]
    fresh = api.Renderer(sc2)
    assert_frame(B, fresh.render(), "the replaced mesh")
    fresh.close()
    assert not np.array_equal(B["packed"], A["packed"])
    assert_blas(r.read_blas(0), mk, "after the replacement")

    sv, verts = soup_of(mk)
    r.bind_blas_vertices(0, sv, len(verts))
    assert_frame(r.render(), B, "after the bind")
    r.refit_blas(0, torch.from_numpy(verts).cuda())
    assert_frame(r.render(), B, "after a refit with the unchanged vertices")
    assert r.read_blas(0).tri_hot.tobytes() == mk.tri_hot.tobytes()

    assert upload_blas(r, 0, sc.blas[0]) == 0                                    # the cube again: the binding goes with the old arrays
    r.set_frame(sc)
    p = torch.from_numpy(verts).cuda()
    assert r.lib.rtx_refit_blas(r.ctx, 0, p.data_ptr(), None, len(verts)) == STATE
    assert_frame(r.render(), A, "the cube again")
    assert_blas(r.read_blas(0), sc.blas[0], "the cube again")
    r.close()


COUNTS = (1, 3, 2, 5, 4)      # five uploads through three slots: slots 0 and 1 come round again, each with more to hold than before


def test_staging_rings_wrap_and_grow(api):
    """Five rtx_set_views, five rtx_set_rays and five rtx_set_frame calls in a row, each followed by its render call: every slot of every ring
    is reused, two of them by an upload larger than the one they were allocated for.  Every view is the single-view frame of its camera."""
    sc = cube_scene()
    cams = camera_set(sc)[:max(COUNTS)]
    singles = []
    r = api.Renderer(sc)
    for cam in cams:
        r.set_frame(with_camera(sc, cam))
        singles.append(r.render())
    r.close()

    r = api.Renderer(sc)
    for n in COUNTS:
        r.set_views(cams[:n])
        out = r.render_views()
        assert out["rgb"].shape[0] == n
        for k in range(n):
            assert_same(out["rgb"][k], singles[k]["rgb"], f"{n} views, view {k} rgb")
            assert_same(out["packed"][k], singles[k]["packed"], f"{n} views, view {k} packed")
    rays = camera_rays(api, sc, cams)
    for n in COUNTS:
        r.set_rays(rays[:n])
        out = r.render_rays()
        assert out["rgb"].shape[0] == n
        for k in range(n):
            assert_same(out["rgb"][k], singles[k]["rgb"], f"{n} ray views, view {k} rgb")
            assert_same(out["packed"][k], singles[k]["packed"], f"{n} ray views, view {k} packed")

    # frames: the cube's, and the same with one more sphere in front of the camera
    more = copy.copy(sc)
    cam = sc.camera[0]
    ahead = (cam["rotated_top_left_corner"] + f32(SIDE / 2) * (cam["rotated_x_axis"] + cam["rotated_y_axis"])).astype(f32)
    ball = np.zeros(1, sc.spheres.dtype)
    ball["center"] = cam["position"] + f32(2.0) * ahead / f32(np.linalg.norm(ahead))
    ball["radius_inv"] = f32(1.0 / 0.25); ball["radius_squared"] = f32(0.25 * 0.25); ball["material_id"] = 1
    more.spheres = np.concatenate([sc.spheres, ball])
    want = []
    for s in (sc, more):
        one = api.Renderer(s); want.append(one.render()); one.close()
    assert not np.array_equal(want[0]["packed"], want[1]["packed"])              # the sphere is in view
    for call in range(5):
        r.set_frame((sc, more)[call % 2])
        assert_frame(r.render(), want[call % 2], f"set_frame call {call}")
    r.close()


def test_aov_growth_keeps_pixels(api):
    """The context's own AOV buffers, depth and object id bound: grown from one view to three, first by a call that writes only views 1-2,
    then by a call over all three.  View 0 reads back what the first call wrote."""
    sc = cube_scene()
    cams = camera_set(sc)[:3]
    names = ("depth", "object_id")
    r = api.Renderer(sc)
    r.set_views(cams)
    r.bind_aovs(names)
    r.render_views_async(0, 1, aov=True)
    first = r.read_aovs(names, 0, 1)
    assert len(np.unique(first["object_id"])) > 1                                # hits and misses: not a buffer of one value
    r.render_views_async(1, 2, aov=True)                                         # grows to three views, writes views 1 and 2
    kept = r.read_aovs(names, 0, 1)
    r.render_views_async(0, 3, aov=True)
    again = r.read_aovs(names, 0, 3)
    for ch in names:
        assert_same(kept[ch], first[ch], f"{ch} of view 0 after the growth")
        assert_same(again[ch][:1], first[ch], f"{ch} of view 0 after the call over three views")
    one = api.Renderer(sc)                                                       # views 1 and 2 are their cameras' own AOVs
    for k in (1, 2):
        one.set_frame(with_camera(sc, cams[k]))
        ref = one.render_aovs(names)
        for ch in names:
            assert_same(again[ch][k], ref[ch], f"{ch} of view {k}")
    one.close()
    r.close()
