"""ctypes binding of librtx_host.so (include/rtx_host.h) and scene construction on top of it.

Host-side only: per-frame Scene::update equivalents, this repo's own BLAS builder, the procedural
cfg3 "atrium" stand-in for the absent Sponza mesh.  Produces pyrtx.scene_io.Scene objects, which
both the product (api.Renderer) and the oracle consume as plain data.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import scene_io as sio
from .ctypes_structs import RtxCamera, RtxTextureDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "..", "host", "librtx_host.so")
EXPORTS = ["rtxh_camera_basis", "rtxh_camera_update", "rtxh_quaternion_axis_angle", "rtxh_scene_dynamic_animate", "rtxh_scene_update", "rtxh_instance_update", "rtxh_plane_update", "rtxh_tlas_create", "rtxh_tlas_destroy",
           "rtxh_tlas_build", "rtxh_blas_build", "rtxh_blas_build_reference_bvh", "rtxh_blas_build_reference_sbvh", "rtxh_texture_mips", "rtxh_query_sort_order", "rtxh_texture_load", "rtxh_texture_free", "rtxh_sky_load", "rtxh_image_load", "rtxh_image_free", "rtxh_image_save_png", "rtxh_atrium_generate", "rtxh_mesh_free",
           "rtxh_obj_load", "rtxh_obj_free", "rtxh_mtl_load", "rtxh_bvh_cache_load", "rtxh_bvh_cache_save", "rtxh_bvh_cache_free",
           "rtxh_tlas_build_balanced", "rtxh_scene_update_balanced", "rtxh_tlas_balanced_node_count", "rtxh_tlas_balanced_inner_depth", "rtxh_blas_refit",
           "rtxh_blas_build_balanced", "rtxh_blas_balanced_node_count", "rtxh_blas_balanced_inner_depth", "rtxh_vertex_normals",
           "rtxh_query_nearest", "rtxh_query_nearest_exhaustive", "rtxh_nearest_distance_bound", "rtxh_nearest_box_d2", "rtxh_nearest_triangle_d2",
           "rtxh_nearest_sphere_d2", "rtxh_nearest_plane_d2", "rtxh_query_hits", "rtxh_query_hits_exhaustive", "rtxh_hits_margin",
           "rtxh_query_sweep", "rtxh_query_sweep_exhaustive", "rtxh_sweep_bound", "rtxh_query_sweep_box", "rtxh_query_sweep_box_exhaustive", "rtxh_sweep_box_bound", "rtxh_sweep_box_triangle", "rtxh_sweep_box_sphere", "rtxh_sweep_box_plane", "rtxh_sweep_triangle", "rtxh_sweep_sphere", "rtxh_sweep_plane",
           "rtxh_query_nearest_filtered", "rtxh_query_nearest_exhaustive_filtered", "rtxh_query_hits_filtered", "rtxh_query_hits_exhaustive_filtered",
           "rtxh_query_sweep_filtered", "rtxh_query_sweep_exhaustive_filtered", "rtxh_blas_pseudonormals",
           "rtxh_query_signed_distance", "rtxh_query_signed_distance_filtered", "rtxh_query_signed_distance_exhaustive", "rtxh_query_signed_distance_exhaustive_filtered",
           "rtxh_query_overlap", "rtxh_query_overlap_exhaustive", "rtxh_query_overlap_filtered", "rtxh_query_overlap_exhaustive_filtered", "rtxh_overlap_margin", "rtxh_instances_rigid",
           "rtxh_query_overlap_capsule", "rtxh_query_overlap_capsule_exhaustive", "rtxh_query_overlap_capsule_filtered", "rtxh_query_overlap_capsule_exhaustive_filtered", "rtxh_capsule_margin"]
FLOAT_EXPORTS = ("rtxh_nearest_distance_bound", "rtxh_nearest_box_d2", "rtxh_nearest_triangle_d2", "rtxh_nearest_sphere_d2", "rtxh_nearest_plane_d2", "rtxh_hits_margin", "rtxh_sweep_bound", "rtxh_overlap_margin", "rtxh_sweep_box_bound", "rtxh_capsule_margin")      # return a float, not a status

PI = np.float32(3.14159265359)          # Util.h:8


class RtxhMesh(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("material_ids", C.POINTER(C.c_int32)), ("triangle_count", C.c_int32), ("material_count", C.c_int32)]


class RtxhObj(C.Structure):
    _fields_ = [("mesh", RtxhMesh), ("materials", C.c_void_p), ("texture_names", C.c_void_p)]


class RtxhBvhCache(C.Structure):
    _fields_ = [("triangle_count", C.c_int32), ("node_count", C.c_int32), ("index_count", C.c_int32), ("pad", C.c_int32),
                ("hot", C.c_void_p), ("cold", C.c_void_p), ("nodes", C.c_void_p), ("indices", C.c_void_p)]


class RtxhNearestBlas(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("hot", C.c_void_p), ("cold", C.c_void_p),
                ("node_count", C.c_int32), ("triangle_count", C.c_int32), ("material_offset", C.c_int32), ("pad", C.c_int32)]


class RtxhNearestScene(C.Structure):
    _fields_ = [("instances", C.c_void_p), ("tlas_nodes", C.c_void_p), ("tlas_indices", C.c_void_p), ("blas", C.POINTER(RtxhNearestBlas)),
                ("spheres", C.c_void_p), ("planes", C.c_void_p),
                ("instance_count", C.c_int32), ("tlas_node_count", C.c_int32), ("tlas_index_count", C.c_int32), ("blas_count", C.c_int32),
                ("sphere_count", C.c_int32), ("plane_count", C.c_int32)]


class RtxhSideBlas(C.Structure):
    _fields_ = [("vert_pn", C.c_void_p), ("edge_pn", C.c_void_p), ("slot_vertices", C.c_void_p), ("vertex_count", C.c_int32), ("pad", C.c_int32)]


TEXNAME_MAX = 512
_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.abspath(LIB_PATH)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: run __graft_entry__.build()")
        l = C.CDLL(path)
        vp, i32 = C.c_void_p, C.c_int32
        l.rtxh_camera_basis.argtypes = [i32, i32, C.c_float, vp, vp, C.POINTER(RtxCamera)]
        l.rtxh_instance_update.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        l.rtxh_plane_update.argtypes = [vp, vp, i32, vp]
        l.rtxh_tlas_create.argtypes = [i32, C.POINTER(vp)]
        l.rtxh_tlas_destroy.argtypes = [vp]
        l.rtxh_tlas_build.argtypes = [vp, vp, vp, vp, vp, C.POINTER(i32)]
        l.rtxh_blas_build.argtypes = [vp, i32, i32, vp, C.POINTER(i32), vp]
        l.rtxh_blas_build_reference_bvh.argtypes = [vp, i32, vp, C.POINTER(i32), vp]
        l.rtxh_quaternion_axis_angle.argtypes = [vp, C.c_float, vp]
        l.rtxh_camera_update.argtypes = [C.c_float, C.c_uint32, vp, vp]
        l.rtxh_scene_dynamic_animate.argtypes = [C.c_float, C.POINTER(C.c_float), vp, vp, i32]
        l.rtxh_scene_update.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
        l.rtxh_texture_load.argtypes = [C.c_char_p, i32, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int64), C.POINTER(RtxTextureDesc)]
        l.rtxh_texture_free.argtypes = [C.POINTER(C.c_float)]
        l.rtxh_sky_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(i32)]
        l.rtxh_image_load.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.POINTER(C.c_uint8))]
        l.rtxh_image_free.argtypes = [C.POINTER(C.c_uint8)]
        l.rtxh_image_save_png.argtypes = [C.c_char_p, vp, i32, i32]
        l.rtxh_blas_build_reference_sbvh.argtypes = [vp, i32, vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32)]
        l.rtxh_obj_load.argtypes = [C.c_char_p, C.POINTER(RtxhObj)]
        l.rtxh_obj_free.argtypes = [C.POINTER(RtxhObj)]
        l.rtxh_mtl_load.argtypes = [C.c_char_p, C.POINTER(RtxhObj)]
        l.rtxh_bvh_cache_load.argtypes = [C.c_char_p, C.POINTER(RtxhBvhCache)]
        l.rtxh_bvh_cache_save.argtypes = [C.c_char_p, C.POINTER(RtxhBvhCache)]
        l.rtxh_bvh_cache_free.argtypes = [C.POINTER(RtxhBvhCache)]
        l.rtxh_texture_mips.argtypes = [vp, i32, i32, C.POINTER(RtxTextureDesc), C.POINTER(C.c_int64)]
        l.rtxh_query_sort_order.argtypes = [vp, i32, C.c_int64, vp]
        l.rtxh_atrium_generate.argtypes = [C.c_uint32, i32, C.POINTER(RtxhMesh)]
        l.rtxh_mesh_free.argtypes = [C.POINTER(RtxhMesh)]
        l.rtxh_tlas_build_balanced.argtypes = [i32, vp, vp, vp, vp, C.POINTER(i32)]
        l.rtxh_scene_update_balanced.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
        l.rtxh_tlas_balanced_node_count.argtypes = [i32]
        l.rtxh_instances_rigid.argtypes = [vp, i32, C.POINTER(C.c_double)]
        l.rtxh_tlas_balanced_inner_depth.argtypes = [i32]
        l.rtxh_blas_refit.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, vp]
        l.rtxh_blas_build_balanced.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, C.POINTER(i32), vp, vp, vp, vp]
        l.rtxh_blas_balanced_node_count.argtypes = [i32]
        l.rtxh_blas_balanced_inner_depth.argtypes = [i32]
        l.rtxh_vertex_normals.argtypes = [vp, vp, i32, i32, vp]
        l.rtxh_query_nearest.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, C.c_uint32, vp, C.POINTER(i32)]
        l.rtxh_query_nearest_exhaustive.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, C.c_uint32, vp]
        l.rtxh_nearest_distance_bound.argtypes = [C.c_float, C.c_float]
        l.rtxh_nearest_box_d2.argtypes = [vp, vp, vp]
        l.rtxh_nearest_triangle_d2.argtypes = [vp, vp, vp]
        l.rtxh_nearest_sphere_d2.argtypes = [vp, vp]
        l.rtxh_nearest_plane_d2.argtypes = [vp, vp]
        l.rtxh_query_hits.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, i32, C.c_uint32, vp, vp, C.POINTER(i32)]
        l.rtxh_query_hits_exhaustive.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, i32, C.c_uint32, vp, vp]
        l.rtxh_hits_margin.argtypes = [C.c_float, C.c_float]
        l.rtxh_query_sweep.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, C.c_uint32, vp, C.POINTER(i32)]
        l.rtxh_query_sweep_exhaustive.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, C.c_uint32, vp]
        masks3 = [vp, vp, C.c_uint32]                              # object_masks, row_masks, row_mask
        l.rtxh_query_nearest_filtered.argtypes = l.rtxh_query_nearest.argtypes + masks3
        l.rtxh_query_nearest_exhaustive_filtered.argtypes = l.rtxh_query_nearest_exhaustive.argtypes + masks3
        l.rtxh_query_hits_filtered.argtypes = l.rtxh_query_hits.argtypes + masks3
        l.rtxh_query_hits_exhaustive_filtered.argtypes = l.rtxh_query_hits_exhaustive.argtypes + masks3
        l.rtxh_query_sweep_filtered.argtypes = l.rtxh_query_sweep.argtypes + masks3
        l.rtxh_query_sweep_exhaustive_filtered.argtypes = l.rtxh_query_sweep_exhaustive.argtypes + masks3
        l.rtxh_blas_pseudonormals.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp]
        side3 = [C.POINTER(RtxhSideBlas), vp, vp]                  # side, signed_out, feature_out
        l.rtxh_query_signed_distance.argtypes = l.rtxh_query_nearest.argtypes[:5] + side3 + [C.POINTER(i32)]
        l.rtxh_query_signed_distance_exhaustive.argtypes = l.rtxh_query_nearest_exhaustive.argtypes[:5] + side3
        l.rtxh_query_signed_distance_filtered.argtypes = l.rtxh_query_signed_distance.argtypes + masks3
        l.rtxh_query_signed_distance_exhaustive_filtered.argtypes = l.rtxh_query_signed_distance_exhaustive.argtypes + masks3
        l.rtxh_query_overlap.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, i32, vp, vp, vp, C.c_uint32, C.POINTER(i32)]
        l.rtxh_query_overlap_exhaustive.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, i32, vp, vp, vp, C.c_uint32]
        l.rtxh_query_overlap_filtered.argtypes = l.rtxh_query_overlap.argtypes + masks3
        l.rtxh_query_overlap_exhaustive_filtered.argtypes = l.rtxh_query_overlap_exhaustive.argtypes + masks3
        l.rtxh_overlap_margin.argtypes = [C.c_float, C.c_float, C.c_float]
        l.rtxh_query_overlap_capsule.argtypes = l.rtxh_query_overlap.argtypes
        l.rtxh_query_overlap_capsule_exhaustive.argtypes = l.rtxh_query_overlap_exhaustive.argtypes
        l.rtxh_query_overlap_capsule_filtered.argtypes = l.rtxh_query_overlap_filtered.argtypes
        l.rtxh_query_overlap_capsule_exhaustive_filtered.argtypes = l.rtxh_query_overlap_exhaustive_filtered.argtypes
        l.rtxh_capsule_margin.argtypes = [C.c_float, C.c_float, C.c_float]
        l.rtxh_sweep_bound.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float]
        l.rtxh_sweep_triangle.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp, vp, vp]
        l.rtxh_sweep_sphere.argtypes = [vp, vp, C.c_float, vp, vp, vp]
        l.rtxh_sweep_plane.argtypes = [vp, vp, C.c_float, vp, vp, vp]
        l.rtxh_query_sweep_box.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, vp, vp, vp, vp, vp, C.POINTER(i32)] + masks3
        l.rtxh_query_sweep_box_exhaustive.argtypes = [C.POINTER(RtxhNearestScene), vp, C.c_int64, vp, vp, vp, vp, vp] + masks3
        l.rtxh_sweep_box_bound.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float]
        l.rtxh_sweep_box_triangle.argtypes = [vp, C.c_float, vp, vp, vp]
        l.rtxh_sweep_box_sphere.argtypes = [vp, C.c_float, vp, vp]
        l.rtxh_sweep_box_plane.argtypes = [vp, vp, vp]
        for n in EXPORTS:
            getattr(l, n).restype = C.c_float if n in FLOAT_EXPORTS else C.c_int
        _lib = l
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def axis_angle(axis: Sequence[float], angle: float) -> np.ndarray:
    """Quaternion::axis_angle, Quaternion.h:24-34 (sinf/cosf in fp32)."""
    out = np.zeros(4, np.float32)
    a = _f32(axis)
    assert lib().rtxh_quaternion_axis_angle(a.ctypes.data, C.c_float(float(np.float32(angle))), out.ctypes.data) == 0
    return out


KEYS = {"W": 1, "A": 2, "S": 4, "D": 8, "LSHIFT": 16, "SPACE": 32, "UP": 64, "DOWN": 128, "LEFT": 256, "RIGHT": 512}   # RTXH_KEY_*


def camera_update(delta: float, keys, position, rotation):
    """Camera::update's keyboard half (Camera.cpp:18-39); keys: iterable of names from KEYS.  Returns (position, rotation)."""
    p, r = _f32(position).copy(), _f32(rotation).copy()
    mask = 0
    for k in keys:
        mask |= KEYS[k]
    assert lib().rtxh_camera_update(C.c_float(float(np.float32(delta))), mask, p.ctypes.data, r.ctypes.data) == 0
    return p, r


def camera_basis(width: int, height: int, fov: float, position, rotation) -> np.ndarray:
    out = RtxCamera()
    p, r = _f32(position), _f32(rotation)
    rc = lib().rtxh_camera_basis(width, height, C.c_float(fov), p.ctypes.data, r.ctypes.data, C.byref(out))
    assert rc == 0
    cam = np.zeros(1, sio.CAMERA)
    C.memmove(cam.ctypes.data, C.byref(out), C.sizeof(out))
    return cam


def instance_update(position, rotation, root_min, root_max, blas_id: int):
    inst = np.zeros(1, sio.INSTANCE)
    mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
    p, r, a, b = _f32(position), _f32(rotation), _f32(root_min), _f32(root_max)
    rc = lib().rtxh_instance_update(p.ctypes.data, r.ctypes.data, a.ctypes.data, b.ctypes.data, inst.ctypes.data, mn.ctypes.data, mx.ctypes.data)
    assert rc == 0
    inst["blas_id"] = blas_id
    return inst, mn, mx


def plane_update(position, rotation, material_id: int) -> np.ndarray:
    out = np.zeros(1, sio.PLANE)
    p, r = _f32(position), _f32(rotation)
    assert lib().rtxh_plane_update(p.ctypes.data, r.ctypes.data, material_id, out.ctypes.data) == 0
    return out


class Tlas:
    """Persistent TLAS builder: TopLevelBVH::init + build_bvh every frame (TopLevelBVH.cpp:5-45)."""

    def __init__(self, n: int):
        self.n = n
        self.h = C.c_void_p()
        assert lib().rtxh_tlas_create(n, C.byref(self.h)) == 0

    def build(self, positions: np.ndarray, aabbs: np.ndarray):
        p, a = _f32(positions).reshape(self.n, 3), _f32(aabbs).reshape(self.n, 6)
        nodes = np.zeros(2 * self.n, sio.BVH_NODE)
        idx = np.zeros(self.n, np.int32)
        nc = C.c_int32()
        assert lib().rtxh_tlas_build(self.h, p.ctypes.data, a.ctypes.data, nodes.ctypes.data, idx.ctypes.data, C.byref(nc)) == 0
        return nodes[:nc.value].copy(), idx

    def __del__(self):
        try:
            lib().rtxh_tlas_destroy(self.h)
        except Exception:
            pass


def instances_rigid(instances, deviation: bool = False):
    """rtxh_instances_rigid: True when every instance's world and world_inv are rigid poses within tau = 2^-12 (csrc/rtx_update_math.h), the
    rule by which rtx_set_frame decides whether the length queries answer.  deviation=True: (rigid, largest |(R.R^T - I)ij|)."""
    inst = np.ascontiguousarray(instances, sio.INSTANCE)
    dev = C.c_double(0.0)
    rigid = lib().rtxh_instances_rigid(inst.ctypes.data if len(inst) else None, len(inst), C.byref(dev)) == 1
    return (rigid, float(dev.value)) if deviation else rigid


def tlas_balanced_node_count(n: int) -> int:
    """Node slots of the balanced TLAS of n instances (2 << ceil(log2 n), holes and index 1 included); 0 outside 1 .. 65 536."""
    return int(lib().rtxh_tlas_balanced_node_count(n))


def tlas_balanced_inner_depth(n: int) -> int:
    """Depth of the deepest inner node of the balanced TLAS of n instances: ceil(log2 n) - 1, -1 for one instance."""
    return int(lib().rtxh_tlas_balanced_inner_depth(n))


def tlas_build_balanced(positions: np.ndarray, aabbs: np.ndarray):
    """rtxh_tlas_build_balanced: the TLAS rtx_update_instances builds on the device, from the same code.  positions (n, 3), aabbs (n, 6)
    -> (BVH_NODE array of tlas_balanced_node_count(n) slots, int32 indices (n,))."""
    p = _f32(positions).reshape(-1, 3)
    n = p.shape[0]
    a = _f32(aabbs).reshape(n, 6)
    slots = tlas_balanced_node_count(n)
    if slots == 0:
        raise ValueError(f"1 .. 65536 instances, not {n}")
    nodes = np.zeros(slots, sio.BVH_NODE)
    idx = np.zeros(n, np.int32)
    nc = C.c_int32()
    rc = lib().rtxh_tlas_build_balanced(n, p.ctypes.data, a.ctypes.data, nodes.ctypes.data, idx.ctypes.data, C.byref(nc))
    if rc:
        raise ValueError(f"rtxh_tlas_build_balanced failed with status {rc}")
    return nodes[:nc.value], idx


def scene_update_balanced(scene: sio.Scene, positions, rotations):
    """rtxh_scene_update_balanced: what Renderer.update_instances(positions, rotations) leaves on the device for `scene` (its BLAS set and the
    blas_id of its instances) -> (instances, tlas_nodes, tlas_indices)."""
    n = len(scene.instances)
    p, r = _f32(positions).reshape(n, 3), _f32(rotations).reshape(n, 4)
    blas_ids = np.ascontiguousarray(scene.instances["blas_id"], np.int32)
    roots = np.concatenate([np.concatenate([b.nodes[0]["aabb_min"], b.nodes[0]["aabb_max"]]) for b in scene.blas]).astype(np.float32)
    inst = np.zeros(n, sio.INSTANCE)
    nodes = np.zeros(tlas_balanced_node_count(n), sio.BVH_NODE)
    idx = np.zeros(n, np.int32)
    nc = C.c_int32()
    rc = lib().rtxh_scene_update_balanced(n, p.ctypes.data, r.ctypes.data, blas_ids.ctypes.data, roots.ctypes.data, inst.ctypes.data,
                                          nodes.ctypes.data, idx.ctypes.data, C.byref(nc))
    if rc:
        raise ValueError(f"rtxh_scene_update_balanced failed with status {rc}")
    return inst, nodes[:nc.value], idx


class DynamicScene:
    """Per-frame state of a scene whose instances move: Scene::update (Scene.cpp:139-171) in two native calls per frame."""

    def __init__(self, scene: sio.Scene, positions, rotations):
        self.n = len(scene.instances)
        self.pos = np.ascontiguousarray(positions, np.float32).reshape(self.n, 3).copy()
        self.rot = np.ascontiguousarray(rotations, np.float32).reshape(self.n, 4).copy()
        self.time = C.c_float(0.0)
        self.blas_ids = np.ascontiguousarray(scene.instances["blas_id"], np.int32)
        self.roots = np.concatenate([np.concatenate([b.nodes[0]["aabb_min"], b.nodes[0]["aabb_max"]]) for b in scene.blas]).astype(np.float32)
        self.tlas = Tlas(self.n)
        self.instances = np.zeros(self.n, sio.INSTANCE)
        self.nodes = np.zeros(2 * self.n, sio.BVH_NODE)
        self.indices = np.zeros(self.n, np.int32)

    def animate_dynamic(self, delta: float):
        assert lib().rtxh_scene_dynamic_animate(C.c_float(delta), C.byref(self.time), self.pos.ctypes.data, self.rot.ctypes.data, self.n) == 0

    def update(self):
        """-> (instances, tlas_nodes, tlas_indices) for rtx_set_frame"""
        nc = C.c_int32()
        rc = lib().rtxh_scene_update(self.tlas.h, self.n, self.pos.ctypes.data, self.rot.ctypes.data, self.blas_ids.ctypes.data, self.roots.ctypes.data,
                                     self.instances.ctypes.data, self.nodes.ctypes.data, self.indices.ctypes.data, C.byref(nc))
        assert rc == 0, rc
        return self.instances, self.nodes[:nc.value], self.indices


def load_obj(path: str):
    """OBJLoader::load_obj equivalent: (positions (n,3,3), normals, texcoords (n,3,2), material ids, MATERIAL array,
    texture path per material or None)."""
    o = RtxhObj()
    rc = lib().rtxh_obj_load(path.encode(), C.byref(o))
    if rc:
        raise RuntimeError(f"rtxh_obj_load({path}) failed: {rc}")
    n, nm = o.mesh.triangle_count, o.mesh.material_count
    pos = np.ctypeslib.as_array(o.mesh.positions, (n, 3, 3)).copy()
    nrm = np.ctypeslib.as_array(o.mesh.normals, (n, 3, 3)).copy()
    uv = np.ctypeslib.as_array(o.mesh.texcoords, (n, 3, 2)).copy()
    mid = np.ctypeslib.as_array(o.mesh.material_ids, (n,)).copy()
    mats = np.frombuffer((C.c_char * (nm * sio.MATERIAL.itemsize)).from_address(o.materials), sio.MATERIAL).copy()
    names_raw = (C.c_char * (nm * TEXNAME_MAX)).from_address(o.texture_names).raw
    names = [names_raw[i * TEXNAME_MAX:(i + 1) * TEXNAME_MAX].split(b"\0")[0].decode() or None for i in range(nm)]
    lib().rtxh_obj_free(C.byref(o))
    return pos, nrm, uv, mid, mats, names


def build_blas(positions: np.ndarray, normals: np.ndarray, texcoords: np.ndarray, material_ids: np.ndarray,
               material_offset: int, bins: int = 32, reference_bvh: bool = False, reference_sbvh: bool = False) -> sio.Blas:
    """Triangle soup (n,3,3) + per-vertex normals (n,3,3) + texcoords (n,3,2) -> flattened BLAS
    (TriangleHot / TriangleCold as OBJLoader.cpp:156-175 fills them, in leaf order as BottomLevelBVH::flatten :196-212)."""
    pos = _f32(positions).reshape(-1, 9)
    n = pos.shape[0]
    nc = C.c_int32()
    if reference_sbvh:    # the reference's default MESH_ACCELERATOR_SBVH topology (BVHBuilders.h:48-329): leaves may share triangles
        cap = 2 * n
        while True:
            nodes = np.zeros(2 * cap, sio.BVH_NODE)
            order = np.zeros(cap, np.int32)
            oc = C.c_int32()
            rc = lib().rtxh_blas_build_reference_sbvh(pos.ctypes.data, n, nodes.ctypes.data, len(nodes), C.byref(nc),
                                                      order.ctypes.data, cap, C.byref(oc))
            if rc != 4 or cap >= 32 * n:   # RTX_ERR_LIMIT: more duplicated references than the reference's own 2n arrays hold
                break                          # (beyond 32n the input is pathological, e.g. piles of coplanar overlapping triangles: give up)
            cap *= 2
        if rc:
            raise ValueError(f"rtxh_blas_build_reference_sbvh failed with status {rc}" + (" (reference explosion: try the plain BVH)" if rc == 4 else ""))
        order = order[:oc.value]
    else:
        nodes = np.zeros(2 * n, sio.BVH_NODE)
        order = np.zeros(n, np.int32)
        if reference_bvh:     # the reference's MESH_ACCELERATOR_BVH topology (BVHBuilders.h:8-46)
            rc = lib().rtxh_blas_build_reference_bvh(pos.ctypes.data, n, nodes.ctypes.data, C.byref(nc), order.ctypes.data)
        else:                 # this repo's binned-SAH builder
            rc = lib().rtxh_blas_build(pos.ctypes.data, n, bins, nodes.ctypes.data, C.byref(nc), order.ctypes.data)
        assert rc == 0, rc
    m = len(order)
    p = pos.reshape(n, 3, 3)[order]
    nr = _f32(normals).reshape(n, 3, 3)[order]
    uv = _f32(texcoords).reshape(n, 3, 2)[order]
    hot = np.zeros(m, sio.TRI_HOT)
    hot["position_0"] = p[:, 0]; hot["position_edge_1"] = p[:, 1] - p[:, 0]; hot["position_edge_2"] = p[:, 2] - p[:, 0]
    cold = np.zeros(m, sio.TRI_COLD)
    cold["tex_coord_0"] = uv[:, 0]; cold["tex_coord_edge_1"] = uv[:, 1] - uv[:, 0]; cold["tex_coord_edge_2"] = uv[:, 2] - uv[:, 0]
    cold["normal_0"] = nr[:, 0]; cold["normal_edge_1"] = nr[:, 1] - nr[:, 0]; cold["normal_edge_2"] = nr[:, 2] - nr[:, 0]
    cold["material_id"] = np.asarray(material_ids, np.int32)[order]
    return sio.Blas(nodes[:nc.value].copy(), hot, cold, material_offset, n, np.ascontiguousarray(order, np.int32).copy())


def slot_vertices(blas: sio.Blas, faces: Optional[np.ndarray] = None) -> np.ndarray:
    """Vertex indices of every flattened slot of a BLAS built by build_blas, int32 (m, 3): for a triangle soup (faces None) vertex c of source
    triangle t is row 3 t + c of the soup's (3 n, 3) positions; for an indexed mesh, faces (n, 3) holds the indices."""
    if blas.order is None:
        raise ValueError("this Blas has no slot order (it was not built by host.build_blas)")
    order = np.asarray(blas.order, np.int64)
    if faces is None:
        return (3 * order[:, None] + np.arange(3)[None, :]).astype(np.int32)
    return np.ascontiguousarray(np.asarray(faces).reshape(-1, 3)[order], np.int32)


def blas_refit(blas: sio.Blas, slot_vertices: np.ndarray, positions: np.ndarray, normals: Optional[np.ndarray] = None) -> sio.Blas:
    """rtxh_blas_refit: the BLAS that Renderer.refit_blas leaves on the device — same topology, hot triangles (and, with normals, the cold
    normals) and every reachable node box recomputed from positions (V, 3) [normals (V, 3)] through slot_vertices (m, 3)."""
    sv = np.ascontiguousarray(slot_vertices, np.int32).reshape(-1, 3)
    pos = _f32(positions).reshape(-1, 3)
    nrm = None if normals is None else _f32(normals).reshape(-1, 3)
    if len(sv) != len(blas.tri_hot):
        raise ValueError(f"slot_vertices holds {len(sv)} slots, the BLAS {len(blas.tri_hot)}")
    if nrm is not None and len(nrm) != len(pos):
        raise ValueError("positions and normals hold different numbers of vertices")
    nodes = np.ascontiguousarray(blas.nodes).copy()
    hot = np.zeros(len(sv), sio.TRI_HOT)
    cold = np.ascontiguousarray(blas.tri_cold).copy()
    rc = lib().rtxh_blas_refit(nodes.ctypes.data, len(nodes), sv.ctypes.data, len(sv), pos.ctypes.data, None if nrm is None else nrm.ctypes.data,
                               len(pos), hot.ctypes.data, cold.ctypes.data)
    if rc:
        raise ValueError(f"rtxh_blas_refit failed with status {rc}")
    return sio.Blas(nodes, hot, cold, blas.material_offset, blas.source_triangle_count, blas.order)


def vertex_normals(positions, indices) -> np.ndarray:
    """rtxh_vertex_normals: the smooth, area-weighted vertex normals (V, 3) that Renderer.vertex_normals writes on the device, from positions
    (V, 3) and indices (T, 3); a triangle with an index outside [0, V) contributes nothing."""
    pos = _f32(positions).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    out = np.zeros((len(pos), 3), np.float32)
    rc = lib().rtxh_vertex_normals(pos.ctypes.data, idx.ctypes.data, len(idx), len(pos), out.ctypes.data)
    if rc:
        raise ValueError(f"rtxh_vertex_normals failed with status {rc}")
    return out


def blas_pseudonormals(positions, indices, slot_vertices):
    """rtxh_blas_pseudonormals: the angle-weighted pseudonormal tables that Renderer.blas_pseudonormals writes on the device (csrc/
    rtx_side_math.h), from positions (V, 3), the SOURCE indices (T, 3) and the slot -> vertex table (slots, 3) of the BLAS (-1: a pad slot)
    -> (vert (V, 4), edge (slots, 3, 4)) float32: per vertex the sum of angle * unit face normal over its corners, per slot edge ab, bc,
    ac the sum of the unit normals of the faces at the edge; w is 0."""
    pos = _f32(positions).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    sv = np.ascontiguousarray(slot_vertices, np.int32).reshape(-1, 3)
    vert = np.zeros((len(pos), 4), np.float32)
    edge = np.zeros((len(sv), 3, 4), np.float32)
    rc = lib().rtxh_blas_pseudonormals(pos.ctypes.data, idx.ctypes.data, len(idx), len(pos), sv.ctypes.data if len(sv) else None, len(sv), vert.ctypes.data,
                                       edge.ctypes.data if len(sv) else None)
    if rc:
        raise ValueError(f"rtxh_blas_pseudonormals failed with status {rc}")
    return vert, edge


def blas_balanced_node_count(n: int) -> int:
    """Node slots of the balanced BLAS of n triangles (2 << L, L the first level with ceil(n / 2^L) <= 4; holes and index 1 included); 0
    outside 1 .. 2^24 - 1."""
    return int(lib().rtxh_blas_balanced_node_count(n))


def blas_balanced_inner_depth(n: int) -> int:
    """Depth of the deepest inner node of the balanced BLAS of n triangles; -1 when the root is a leaf."""
    return int(lib().rtxh_blas_balanced_inner_depth(n))


def blas_build_balanced(positions, indices, normals, texcoords=None, material_ids=None, material_offset: int = 0):
    """rtxh_blas_build_balanced: the BLAS Renderer.alloc_blas + build_blas leave on the device, from the same code.  positions (V, 3),
    indices (T, 3) int32 (a triangle with an index outside [0, V) is invalid), normals (V, 3), texcoords (V, 2) or None, material_ids (T,) or
    None -> (Blas, slot_vertices int32 (T, 3) with -1 -1 -1 for invalid triangles, order int32 (T,))."""
    pos = _f32(positions).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    nrm = _f32(normals).reshape(-1, 3)
    V, T = len(pos), len(idx)
    if len(nrm) != V:
        raise ValueError("positions and normals hold different numbers of vertices")
    uv = None if texcoords is None else _f32(texcoords).reshape(V, 2)
    mid = None if material_ids is None else np.ascontiguousarray(material_ids, np.int32).reshape(T)
    slots = blas_balanced_node_count(T)
    if slots == 0:
        raise ValueError(f"1 .. 2^24 - 1 triangles, not {T}")
    nodes = np.zeros(slots, sio.BVH_NODE); hot = np.zeros(T, sio.TRI_HOT); cold = np.zeros(T, sio.TRI_COLD)
    order = np.zeros(T, np.int32); sv = np.zeros((T, 3), np.int32)
    nc = C.c_int32()
    rc = lib().rtxh_blas_build_balanced(pos.ctypes.data, idx.ctypes.data, nrm.ctypes.data, None if uv is None else uv.ctypes.data,
                                        None if mid is None else mid.ctypes.data, T, V, nodes.ctypes.data, C.byref(nc), hot.ctypes.data,
                                        cold.ctypes.data, order.ctypes.data, sv.ctypes.data)
    if rc:
        raise ValueError(f"rtxh_blas_build_balanced failed with status {rc}")
    return sio.Blas(nodes[:nc.value], hot, cold, material_offset, T, order.copy()), sv, order


def load_bvh_cache(path: str, material_offset: int = 0) -> sio.Blas:
    """Reads a `<mesh>.obj.bvh` file exactly as BottomLevelBVH::load_from_disk does (BottomLevelBVH.cpp:171-192:
    int triangle_count; TriangleHot[n]; TriangleCold[n]; int node_count; BVHNode[node_count]; int index_count; int[index_count])
    and applies BottomLevelBVH::flatten (:196-212).  The record layouts are the C ABI's, so no conversion happens."""
    buf = open(path, "rb").read()
    n = int(np.frombuffer(buf, np.int32, 1, 0)[0]); off = 4
    hot = np.frombuffer(buf, sio.TRI_HOT, n, off); off += n * sio.TRI_HOT.itemsize
    cold = np.frombuffer(buf, sio.TRI_COLD, n, off); off += n * sio.TRI_COLD.itemsize
    nc = int(np.frombuffer(buf, np.int32, 1, off)[0]); off += 4
    nodes = np.frombuffer(buf, sio.BVH_NODE, nc, off).copy(); off += nc * sio.BVH_NODE.itemsize
    ic = int(np.frombuffer(buf, np.int32, 1, off)[0]); off += 4
    idx = np.frombuffer(buf, np.int32, ic, off)
    assert off + 4 * ic == len(buf), "trailing bytes in .bvh cache"
    if nc > 1:
        nodes[1] = np.zeros(1, sio.BVH_NODE)[0]           # never written by the reference (uninitialised heap in the file)
    return sio.Blas(nodes, hot[idx].copy(), cold[idx].copy(), material_offset, n)


def load_bvh_cache_native(path: str, material_offset: int = 0, keep_node1: bool = False) -> sio.Blas:
    """The same file through librtx_host's rtxh_bvh_cache_load (the C / C++ route), flattened like BottomLevelBVH::flatten."""
    c = RtxhBvhCache()
    rc = lib().rtxh_bvh_cache_load(path.encode(), C.byref(c))
    if rc:
        raise ValueError(f"rtxh_bvh_cache_load({path!r}) failed with status {rc}")
    def arr(ptr, dtype, n):
        return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(ptr), dtype, n).copy()
    hot = arr(c.hot, sio.TRI_HOT, c.triangle_count); cold = arr(c.cold, sio.TRI_COLD, c.triangle_count)
    nodes = arr(c.nodes, sio.BVH_NODE, c.node_count); idx = arr(c.indices, np.dtype(np.int32), c.index_count)
    n = c.triangle_count
    lib().rtxh_bvh_cache_free(C.byref(c))
    if len(nodes) > 1 and not keep_node1:
        nodes[1] = np.zeros(1, sio.BVH_NODE)[0]
    return sio.Blas(nodes, hot[idx].copy(), cold[idx].copy(), material_offset, n)


def save_bvh_cache(path: str, blas: sio.Blas) -> None:
    """Writes a flattened BLAS in the reference's `.bvh` layout (BottomLevelBVH.cpp:149-168) with an identity index list,
    so the reference's load_from_disk + flatten reproduce the same arrays."""
    n = len(blas.tri_hot)
    with open(path, "wb") as f:
        f.write(np.int32(n).tobytes()); f.write(np.ascontiguousarray(blas.tri_hot).tobytes()); f.write(np.ascontiguousarray(blas.tri_cold).tobytes())
        f.write(np.int32(len(blas.nodes)).tobytes()); f.write(np.ascontiguousarray(blas.nodes).tobytes())
        f.write(np.int32(n).tobytes()); f.write(np.arange(n, dtype=np.int32).tobytes())


def query_sort_order(rows: np.ndarray) -> np.ndarray:
    """The order Renderer.query_closest / query_occluded trace rows in with sort=True (rtxh_query_sort_order, the code of
    csrc/rtx_query_sort_math.h on the host): rows (n, 6) rays, (n, 7) segments or (n, 4) points of query_nearest, float32 -> int32 (n,),
    element first + i = the row in slot i of the round that starts at row `first`."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] not in (4, 6, 7) or rows.shape[0] < 1:
        raise ValueError(f"rows must have shape (n, 4), (n, 6) or (n, 7) with n >= 1, not {rows.shape}")
    if rows.dtype != np.float32:
        raise TypeError(f"rows must be float32, not {rows.dtype}")
    rows = np.ascontiguousarray(rows)
    order = np.empty(rows.shape[0], np.int32)
    rc = lib().rtxh_query_sort_order(rows.ctypes.data, rows.shape[1], rows.shape[0], order.ctypes.data)
    if rc:
        raise RuntimeError(f"rtxh_query_sort_order failed: {rc}")
    return order


# ---- nearest-point queries on the host (include/rtx_host.h: rtxh_query_nearest / rtxh_query_nearest_exhaustive) ---------------------------
NEAREST_CHANNELS = {"distance": (1, np.float32, 1), "position": (2, np.float32, 3), "normal": (4, np.float32, 3), "uv": (16, np.float32, 2),
                    "material_id": (32, np.int32, 1), "object_id": (64, np.int32, 1), "triangle_id": (128, np.int32, 1)}      # rtx_query_buffers order


class _NearestBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in NEAREST_CHANNELS]


def nearest_scene(scene, blas=None):
    """The arrays a nearest-point query reads, as (RtxhNearestScene, keep-alive list): scene = a scene_io.Scene, or a tuple / dict
    (instances, tlas_nodes, tlas_indices[, spheres, planes]) as Renderer.read_frame_state() returns them, with blas = the list of
    scene_io.Blas from Renderer.read_blas()."""
    if isinstance(scene, sio.Scene):
        inst, nodes, idx, spheres, planes = scene.instances, scene.tlas_nodes, scene.tlas_indices, scene.spheres, scene.planes
        blas = scene.blas if blas is None else blas
    else:
        if isinstance(scene, dict):
            scene = (scene["instances"], scene["tlas_nodes"], scene["tlas_indices"], scene.get("spheres"), scene.get("planes"))
        inst, nodes, idx = scene[0], scene[1], scene[2]
        spheres = scene[3] if len(scene) > 3 and scene[3] is not None else np.zeros(0, sio.SPHERE)
        planes = scene[4] if len(scene) > 4 and scene[4] is not None else np.zeros(0, sio.PLANE)
        if blas is None:
            raise ValueError("frame-state arrays need blas = the list of scene_io.Blas")
    arr = lambda a, dt: np.ascontiguousarray(a, dt)
    inst, nodes, idx = arr(inst, sio.INSTANCE), arr(nodes, sio.BVH_NODE), arr(idx, np.int32)
    spheres, planes = arr(spheres, sio.SPHERE), arr(planes, sio.PLANE)
    keep = [inst, nodes, idx, spheres, planes]
    table = (RtxhNearestBlas * max(1, len(blas)))()
    for b, bl in enumerate(blas):
        n, h, c = arr(bl.nodes, sio.BVH_NODE), arr(bl.tri_hot, sio.TRI_HOT), arr(bl.tri_cold, sio.TRI_COLD)
        keep += [n, h, c]
        table[b] = RtxhNearestBlas(n.ctypes.data, h.ctypes.data, c.ctypes.data, len(n), len(h), int(bl.material_offset), 0)
    keep.append(table)
    ptr = lambda a: a.ctypes.data if len(a) else None
    s = RtxhNearestScene(ptr(inst), ptr(nodes), ptr(idx), table, ptr(spheres), ptr(planes), len(inst), len(nodes), len(idx), len(blas), len(spheres), len(planes))
    return s, keep


def _nearest_names(channels):
    if isinstance(channels, (int, np.integer)) and not isinstance(channels, bool):
        if int(channels) & ~247 or int(channels) <= 0:
            raise ValueError(f"channel mask {channels} must be a non-empty subset of RTX_QUERY_ALL")
        return tuple(n for n, (bit, _, _) in NEAREST_CHANNELS.items() if int(channels) & bit)
    if isinstance(channels, str):
        channels = (channels,)
    want = set(channels)
    bad = [n for n in want if n not in NEAREST_CHANNELS]
    if bad or not want:
        raise ValueError(f"channels must be names out of {', '.join(NEAREST_CHANNELS)}, at least one; not {sorted(map(str, want))}")
    return tuple(n for n in NEAREST_CHANNELS if n in want)


def _mask_bits(name, a, n):
    """n masks as a contiguous uint32 array: int32 and uint32 are both accepted and the bits taken as they are."""
    a = np.asarray(a)
    if a.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
        raise TypeError(f"{name} must be int32 or uint32, not {a.dtype}")
    if a.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), not {a.shape}")
    return np.ascontiguousarray(a).view(np.uint32)


def _filter_args(s, n, mask, object_masks):
    """None (the unfiltered call: mask and object_masks both None) or the three trailing arguments of a rtxh_*_filtered function and
    what keeps them alive.  mask: an int (every row), or n row masks; None with object_masks = all ones."""
    if mask is None and object_masks is None:
        return None
    keep = []
    optr = rptr = None
    scalar = 0xFFFFFFFF
    if object_masks is not None:
        om = _mask_bits("object_masks", object_masks, s.instance_count + s.sphere_count + s.plane_count)
        keep.append(om); optr = om.ctypes.data if len(om) else None
    if mask is not None:
        if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool):
            if not -(1 << 31) <= int(mask) <= 0xFFFFFFFF:
                raise ValueError(f"mask {mask} does not fit 32 bits")
            scalar = int(mask) & 0xFFFFFFFF
        else:
            rm = _mask_bits("mask", mask, n)
            keep.append(rm); rptr = rm.ctypes.data
    return [optr, rptr, scalar], keep


def _side_table(blas_count, pseudonormals, slot_vertices):
    """The rtxh_side_blas array of a signed query: pseudonormals = {blas_id: (vert, edge)} or {blas_id: (vert, edge, slot_vertices)};
    slot_vertices = {blas_id: (slots, 3) int32} for the two-element form.  A mesh without an entry has no tables."""
    table = (RtxhSideBlas * max(1, blas_count))()
    keep = [table]
    for b, rec in (pseudonormals or {}).items():
        if not 0 <= int(b) < blas_count:
            raise ValueError(f"pseudonormals names BLAS {b}, the scene has {blas_count}")
        sv = rec[2] if len(rec) > 2 else (slot_vertices or {}).get(b)
        if sv is None:
            raise ValueError(f"pseudonormals[{b}] needs the slot -> vertex table: (vert, edge, slot_vertices)")
        vert, edge, sv = _f32(rec[0]).reshape(-1, 4), _f32(rec[1]).reshape(-1, 4), np.ascontiguousarray(sv, np.int32).reshape(-1, 3)
        if len(edge) != 3 * len(sv):
            raise ValueError(f"pseudonormals[{b}]: edge holds {len(edge)} records, slot_vertices {len(sv)} slots")
        keep += [vert, edge, sv]
        table[int(b)] = RtxhSideBlas(vert.ctypes.data, edge.ctypes.data, sv.ctypes.data, len(vert), 0)
    return table, keep


def _query_nearest(fn_name, scene, points, channels, blas, with_stack, width=4, label="points", mask=None, object_masks=None, signed=None):
    pts = np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != width or pts.shape[0] < 1:
        raise ValueError(f"{label} must have shape (n, {width}) with n >= 1, not {pts.shape}")
    if pts.dtype != np.float32:
        raise TypeError(f"{label} must be float32, not {pts.dtype}")
    pts = np.ascontiguousarray(pts)
    scalar = isinstance(channels, (str, int, np.integer))
    empty = signed is not None and (channels is None or (not scalar and len(channels) == 0) or (scalar and not isinstance(channels, (str, bool)) and int(channels) == 0))
    names = () if empty else _nearest_names(channels)          # a signed query may ask for no channel
    s, keep = nearest_scene(scene, blas)
    n = pts.shape[0]
    out = {name: np.zeros((n, NEAREST_CHANNELS[name][2]) if NEAREST_CHANNELS[name][2] > 1 else (n,), NEAREST_CHANNELS[name][1]) for name in names}
    buf = _NearestBuffers()
    for name in names:
        setattr(buf, name, out[name].ctypes.data)
    bits = sum(NEAREST_CHANNELS[name][0] for name in names)
    high = C.c_int32(0)
    filt = _filter_args(s, n, mask, object_masks)
    args = [C.byref(s), pts.ctypes.data, n, bits, C.byref(buf)]
    if signed is not None:
        table, keep_side = _side_table(s.blas_count, signed.get("pseudonormals"), signed.get("slot_vertices"))
        out["signed_distance"] = np.zeros(n, np.float32)
        if signed.get("feature", True):
            out["feature"] = np.zeros(n, np.int32)
        args += [table, out["signed_distance"].ctypes.data, out["feature"].ctypes.data if "feature" in out else None]
    args += [C.byref(high)] if with_stack else []
    if filt:
        fn_name += "_filtered"
        args += filt[0]
    rc = getattr(lib(), fn_name)(*args)
    if rc:
        raise ValueError(f"{fn_name} failed with status {rc}")
    if with_stack:
        out["stack_max"] = int(high.value)
    return out


def query_nearest(scene, points, channels=("distance",), blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_nearest: what Renderer.query_nearest writes on the device for points float32 (n, 4) of (x, y, z, maximum distance), from the
    same code (csrc/rtx_nearest_math.h) -> {channel: array} plus "stack_max", the most stack entries a row held.  scene: a scene_io.Scene,
    or the arrays of Renderer.read_frame_state() (+ spheres, planes) with blas = [Renderer.read_blas(b), ...]: see nearest_scene.
    mask / object_masks (here and on the other five query functions below): the filtered form (rtxh_*_filtered) — object_masks = the M
    masks of the objects, instances then spheres then planes (None: all ones), mask = an int for every row or n row masks (None with
    object_masks: all ones); int32 or uint32, the bits as they are.  Both None: the unfiltered call."""
    return _query_nearest("rtxh_query_nearest", scene, points, channels, blas, True, mask=mask, object_masks=object_masks)


def query_nearest_exhaustive(scene, points, channels=("distance",), blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_nearest_exhaustive: the same candidate functions over every primitive, no tree; ties to the lowest (kind, object, slot)."""
    return _query_nearest("rtxh_query_nearest_exhaustive", scene, points, channels, blas, False, mask=mask, object_masks=object_masks)


def query_signed_distance(scene, points, channels=(), blas=None, pseudonormals=None, mask=None, object_masks=None, feature=True, slot_vertices=None,
                          exhaustive=False) -> dict:
    """rtxh_query_signed_distance: what Renderer.query_signed_distance writes on the device -> {"signed_distance": (n,) f32, "feature":
    (n,) i32 (feature=True), channel: array ..., "stack_max"}.  pseudonormals = {blas_id: (vert, edge, slot_vertices)} — the tables of
    blas_pseudonormals or Renderer.read_blas_pseudonormals and the slot -> vertex table they were made with (or (vert, edge) with
    slot_vertices = {blas_id: table}); a mesh without an entry has no tables: feature + 8, the naive face rule.  channels may be empty.
    exhaustive=True: rtxh_query_signed_distance_exhaustive, the search without a tree.
    The slot -> vertex table is part of every entry because a vertex-region lookup goes through it and a scene_io.Blas does not carry it:
    a bare (vert, edge) — what Renderer.read_blas_pseudonormals returns — is not enough on its own and raises a ValueError unless
    slot_vertices= supplies the table; append it, read_blas_pseudonormals(b) + (slot_vertices_b,), as the GPU tests do."""
    sg = {"pseudonormals": pseudonormals, "slot_vertices": slot_vertices, "feature": feature}
    name = "rtxh_query_signed_distance_exhaustive" if exhaustive else "rtxh_query_signed_distance"
    return _query_nearest(name, scene, points, channels, blas, not exhaustive, mask=mask, object_masks=object_masks, signed=sg)


# ---- all-hits segment queries on the host (include/rtx_host.h: rtxh_query_hits / rtxh_query_hits_exhaustive) ------------------------------
def _query_hits(fn_name, scene, segments, max_hits, channels, count, blas, with_stack, mask=None, object_masks=None):
    seg = np.asarray(segments)
    if seg.ndim != 2 or seg.shape[1] != 7 or seg.shape[0] < 1:
        raise ValueError(f"segments must have shape (n, 7) with n >= 1, not {seg.shape}")
    if seg.dtype != np.float32:
        raise TypeError(f"segments must be float32, not {seg.dtype}")
    seg = np.ascontiguousarray(seg)
    K = int(max_hits)
    if not 0 <= K <= 8:
        raise ValueError(f"max_hits must be in [0, 8], not {max_hits}")
    if K == 0:
        if not count or (not isinstance(channels, (str, int, np.integer)) and len(tuple(channels))) or (isinstance(channels, (str, int, np.integer)) and channels):
            raise ValueError("max_hits=0 is the count-only form: channels=() and count=True")
        names = ()
    else:
        names = _nearest_names(channels)
    s, keep = nearest_scene(scene, blas)
    n = seg.shape[0]
    out = {name: np.zeros((n, K, NEAREST_CHANNELS[name][2]) if NEAREST_CHANNELS[name][2] > 1 else (n, K), NEAREST_CHANNELS[name][1]) for name in names}
    buf = _NearestBuffers()
    for name in names:
        setattr(buf, name, out[name].ctypes.data)
    bits = sum(NEAREST_CHANNELS[name][0] for name in names)
    cnt = np.zeros(n, np.int32) if count else None
    cptr = cnt.ctypes.data if count else None
    high = C.c_int32(0)
    filt = _filter_args(s, n, mask, object_masks)
    args = [C.byref(s), seg.ctypes.data, n, K, bits, C.byref(buf), cptr] + ([C.byref(high)] if with_stack else [])
    if filt:
        fn_name += "_filtered"
        args += filt[0]
    rc = getattr(lib(), fn_name)(*args)
    if rc:
        raise ValueError(f"{fn_name} failed with status {rc}")
    if count:
        out["count"] = cnt
    if with_stack:
        out["stack_max"] = int(high.value)
    return out


def query_hits(scene, segments, max_hits=4, channels=("distance",), count=True, blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_hits: what Renderer.query_hits writes on the device for segments float32 (n, 7) of (origin, direction, max distance), from
    the same code (csrc/rtx_hits_math.h) -> {channel: (n, K[, k]) array} plus "count" (n,) int32 if count, plus "stack_max".  max_hits=0 with
    channels=() is the count-only form.  scene and blas as for query_nearest."""
    return _query_hits("rtxh_query_hits", scene, segments, max_hits, channels, count, blas, True, mask, object_masks)


def query_hits_exhaustive(scene, segments, max_hits=4, channels=("distance",), count=True, blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_hits_exhaustive: the same hit tests over every primitive with no box test, the same order rule; "count" = all hits."""
    return _query_hits("rtxh_query_hits_exhaustive", scene, segments, max_hits, channels, count, blas, False, mask, object_masks)


# ---- swept-sphere queries on the host (include/rtx_host.h: rtxh_query_sweep / rtxh_query_sweep_exhaustive) ---------------------------------
def query_sweep(scene, sweeps, channels=("distance",), blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_sweep: what Renderer.query_sweep writes on the device for sweeps float32 (n, 8) of (origin, direction, max distance,
    radius), from the same code (csrc/rtx_sweep_math.h) -> {channel: array} plus "stack_max".  scene and blas as for query_nearest."""
    return _query_nearest("rtxh_query_sweep", scene, sweeps, channels, blas, True, 8, "sweeps", mask, object_masks)


def query_sweep_exhaustive(scene, sweeps, channels=("distance",), blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_sweep_exhaustive: the same candidate functions over every primitive with no box test, the same order rule."""
    return _query_nearest("rtxh_query_sweep_exhaustive", scene, sweeps, channels, blas, False, 8, "sweeps", mask, object_masks)


# ---- swept-box queries on the host (include/rtx_host.h: rtxh_query_sweep_box / rtxh_query_sweep_box_exhaustive) ---------------------------
SWEEP_BOX_CHANNELS = {"distance": (np.float32, 1), "normal": (np.float32, 3), "object_id": (np.int32, 1), "triangle_id": (np.int32, 1), "axis": (np.int32, 1)}


def _query_sweep_box(scene, sweeps, channels, blas, exhaustive, mask, object_masks):
    sw = np.asarray(sweeps)
    if sw.ndim != 2 or sw.shape[1] != 14 or sw.shape[0] < 1:
        raise ValueError(f"sweeps must have shape (n, 14) with n >= 1, not {sw.shape}")
    if sw.dtype != np.float32:
        raise TypeError(f"sweeps must be float32, not {sw.dtype}")
    sw = np.ascontiguousarray(sw)
    names = (channels,) if isinstance(channels, str) else tuple(channels)
    if not names or any(name not in SWEEP_BOX_CHANNELS for name in names):
        raise ValueError(f"channels must be a non-empty subset of {tuple(SWEEP_BOX_CHANNELS)}, not {channels!r}")
    s, keep = nearest_scene(scene, blas)
    n = sw.shape[0]
    out = {name: np.zeros((n, SWEEP_BOX_CHANNELS[name][1]) if SWEEP_BOX_CHANNELS[name][1] > 1 else (n,), SWEEP_BOX_CHANNELS[name][0]) for name in names}
    ptr = lambda name: out[name].ctypes.data if name in out else None
    high = C.c_int32(0)
    filt = _filter_args(s, n, mask, object_masks)
    masks = filt[0] if filt else [None, None, 0xFFFFFFFF]
    args = [C.byref(s), sw.ctypes.data, n, ptr("distance"), ptr("normal"), ptr("object_id"), ptr("triangle_id"), ptr("axis")] + ([] if exhaustive else [C.byref(high)]) + masks
    fn_name = "rtxh_query_sweep_box_exhaustive" if exhaustive else "rtxh_query_sweep_box"
    rc = getattr(lib(), fn_name)(*args)
    if rc:
        raise ValueError(f"{fn_name} failed with status {rc}")
    if not exhaustive:
        out["stack_max"] = int(high.value)
    return out


def query_sweep_box(scene, sweeps, channels=("distance",), blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_sweep_box: what Renderer.query_sweep_box writes on the device for sweeps float32 (n, 14) of (centre, direction, max distance,
    half extents, quaternion x y z w), from the same code (csrc/rtx_boxsweep_math.h) -> {channel: array} over distance, normal, object_id,
    triangle_id, axis, plus "stack_max".  scene and blas as for query_nearest, mask / object_masks as there."""
    return _query_sweep_box(scene, sweeps, channels, blas, False, mask, object_masks)


def query_sweep_box_exhaustive(scene, sweeps, channels=("distance",), blas=None, mask=None, object_masks=None) -> dict:
    """rtxh_query_sweep_box_exhaustive: the same candidate functions over every primitive with no node test, the same order rule."""
    return _query_sweep_box(scene, sweeps, channels, blas, True, mask, object_masks)


def sweep_box_bound(local_scale, world_scale=0.0, travelled=0.0, kappa=1.0) -> float:
    """rtxbs::sweep_box_bound of csrc/rtx_boxsweep_math.h: how far, as a normalised gap, a returned contact may lie from touching exactly."""
    return float(lib().rtxh_sweep_box_bound(C.c_float(float(local_scale)), C.c_float(float(world_scale)), C.c_float(float(travelled)), C.c_float(float(kappa))))


# ---- box-overlap queries on the host (include/rtx_host.h: rtxh_query_overlap / rtxh_query_overlap_exhaustive) -----------------------------
RTX_OVERLAP_OBJECTS = 512
RTX_OVERLAP_ANY = 1024


def _query_overlap(scene, boxes, max_hits, count, objects, any_form, blas, exhaustive, mask, object_masks, rows="boxes", width=10, call="rtxh_query_overlap"):
    bx = np.asarray(boxes)
    if bx.ndim != 2 or bx.shape[1] != width or bx.shape[0] < 1:
        raise ValueError(f"{rows} must have shape (n, {width}) with n >= 1, not {bx.shape}")
    if bx.dtype != np.float32:
        raise TypeError(f"{rows} must be float32, not {bx.dtype}")
    bx = np.ascontiguousarray(bx)
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
        raise TypeError(f"max_hits must be an int, not {type(max_hits).__name__}")
    K = int(max_hits)
    if not 0 <= K <= 8:
        raise ValueError(f"max_hits must be in [0, 8], not {max_hits}")
    if K == 0 and not count:
        raise ValueError("max_hits=0 is the count-only form: count must be True")
    s, keep = nearest_scene(scene, blas)
    n = bx.shape[0]
    out = {}
    if K > 0:
        out["object_id"] = np.zeros((n, K), np.int32)
        if not objects:
            out["triangle_id"] = np.zeros((n, K), np.int32)
    cnt = np.zeros(n, np.int32) if count else None
    flags = RTX_OVERLAP_ANY if any_form else RTX_OVERLAP_OBJECTS if objects else 0
    high = C.c_int32(0)
    filt = _filter_args(s, n, mask, object_masks)
    ptr = lambda name: out[name].ctypes.data if name in out else None
    args = [C.byref(s), bx.ctypes.data, n, K, ptr("object_id"), ptr("triangle_id"), cnt.ctypes.data if count else None, flags] + ([] if exhaustive else [C.byref(high)])
    fn_name = call + "_exhaustive" if exhaustive else call
    if filt:
        fn_name += "_filtered"
        args += filt[0]
    rc = getattr(lib(), fn_name)(*args)
    if rc:
        raise ValueError(f"{fn_name} failed with status {rc}")
    if count:
        out["count"] = cnt
    if not exhaustive:
        out["stack_max"] = int(high.value)
    return out


def query_overlap(scene, boxes, max_hits=4, count=True, objects=False, blas=None, exhaustive=False, mask=None, object_masks=None) -> dict:
    """rtxh_query_overlap: what Renderer.query_overlap writes on the device for boxes float32 (n, 10) of (centre, half extents, quaternion
    x y z w), from the same code (csrc/rtx_overlap_math.h) -> {"object_id": (n, K), "triangle_id": (n, K) (absent with objects=True),
    "count": (n,) if count, "stack_max"}; max_hits=0 gives the count alone.  exhaustive=True: rtxh_query_overlap_exhaustive, every primitive
    with no node test (no "stack_max").  scene and blas as for query_nearest, mask / object_masks as there."""
    return _query_overlap(scene, boxes, max_hits, count, bool(objects), False, blas, bool(exhaustive), mask, object_masks)


def query_overlapped(scene, boxes, blas=None, exhaustive=False, mask=None, object_masks=None) -> np.ndarray:
    """The ANY form (RTX_OVERLAP_ANY): int32 (n,) of 0 / 1, what Renderer.query_overlapped writes."""
    return _query_overlap(scene, boxes, 0, True, False, True, blas, bool(exhaustive), mask, object_masks)["count"]


def overlap_margin(local_scale, world_scale=0.0, kappa=1.0) -> float:
    """rtxop::margin of csrc/rtx_overlap_math.h: how far, as a distance, the computed triangle test may be from the exact one on an axis of
    conditioning kappa."""
    return float(lib().rtxh_overlap_margin(C.c_float(float(local_scale)), C.c_float(float(world_scale)), C.c_float(float(kappa))))


# ---- capsule-overlap queries on the host (include/rtx_host.h: rtxh_query_overlap_capsule / rtxh_query_overlap_capsule_exhaustive) ---------
def query_overlap_capsule(scene, capsules, max_hits=4, count=True, objects=False, blas=None, exhaustive=False, mask=None, object_masks=None) -> dict:
    """rtxh_query_overlap_capsule: what Renderer.query_overlap_capsule writes on the device for capsules float32 (n, 7) of (start point, axis
    vector, radius), from the same code (csrc/rtx_capsule_math.h); the result and the arguments are query_overlap's."""
    return _query_overlap(scene, capsules, max_hits, count, bool(objects), False, blas, bool(exhaustive), mask, object_masks, "capsules", 7, "rtxh_query_overlap_capsule")


def query_overlapped_capsule(scene, capsules, blas=None, exhaustive=False, mask=None, object_masks=None) -> np.ndarray:
    """The ANY form (RTX_OVERLAP_ANY): int32 (n,) of 0 / 1, what Renderer.query_overlapped_capsule writes."""
    return _query_overlap(scene, capsules, 0, True, False, True, blas, bool(exhaustive), mask, object_masks, "capsules", 7, "rtxh_query_overlap_capsule")["count"]


def capsule_margin(local_scale, world_scale=0.0, kappa=1.0) -> float:
    """rtxcp::margin of csrc/rtx_capsule_math.h: how far, as a distance, the computed triangle test may be from the exact one for a sub-test
    of conditioning kappa."""
    return float(lib().rtxh_capsule_margin(C.c_float(float(local_scale)), C.c_float(float(world_scale)), C.c_float(float(kappa))))


def sweep_bound(local_scale, world_scale=0.0, travelled=0.0, radius=0.0) -> float:
    """rtxsp::sweep_bound of csrc/rtx_sweep_math.h: how far, in distance, a returned contact may lie from touching exactly."""
    return float(lib().rtxh_sweep_bound(C.c_float(float(local_scale)), C.c_float(float(world_scale)), C.c_float(float(travelled)), C.c_float(float(radius))))


def hits_margin(kappa, scale) -> float:
    """rtxhp::margin of csrc/rtx_hits_math.h: how far tri_test's u, v, t may lie from their exact values (linear in both arguments)."""
    return float(lib().rtxh_hits_margin(C.c_float(float(kappa)), C.c_float(float(scale))))


def nearest_distance_bound(local_scale, world_scale=0.0) -> float:
    """rtxnp::distance_bound of csrc/rtx_nearest_math.h: how far the walk's distance may exceed the exhaustive minimum."""
    return float(lib().rtxh_nearest_distance_bound(C.c_float(float(local_scale)), C.c_float(float(world_scale))))


def texture_with_mips(level0_rgb: np.ndarray) -> sio.Texture:
    """level0_rgb: (h, w, 3) linear-space float32 -> Texture with the reference's box-filter chain."""
    h, w, _ = level0_rgb.shape
    buf = np.zeros((w * h + (w * h) // 3 + 2, 3), np.float32)
    buf[:w * h] = level0_rgb.reshape(-1, 3)
    desc = RtxTextureDesc()
    cnt = C.c_int64()
    assert lib().rtxh_texture_mips(buf.ctypes.data, w, h, C.byref(desc), C.byref(cnt)) == 0
    d = np.zeros(1, sio.TEXTURE_DESC)
    C.memmove(d.ctypes.data, C.byref(desc), C.sizeof(desc))
    return sio.Texture(d, buf[:cnt.value].copy())


def load_image(path: str) -> np.ndarray:
    """PNG / TGA file -> (h, w, 4) uint8 RGBA, decoded like stbi_load(..., STBI_rgb_alpha) at Texture.cpp:40."""
    w = C.c_int32(); h = C.c_int32(); p = C.POINTER(C.c_uint8)()
    rc = lib().rtxh_image_load(path.encode(), C.byref(w), C.byref(h), C.byref(p))
    if rc:
        raise ValueError(f"rtxh_image_load({path!r}) failed with status {rc}")
    out = np.ctypeslib.as_array(p, (h.value, w.value, 4)).copy()
    lib().rtxh_image_free(p)
    return out


def load_sky(path: str) -> np.ndarray:
    """Sky::Sky (Sky.cpp:8-26): raw float3 probe file -> (size, size, 3) float32."""
    p = C.POINTER(C.c_float)(); n = C.c_int32()
    rc = lib().rtxh_sky_load(path.encode(), C.byref(p), C.byref(n))
    if rc:
        raise ValueError(f"rtxh_sky_load({path!r}) failed with status {rc}")
    out = np.ctypeslib.as_array(p, (n.value, n.value, 3)).copy()
    lib().rtxh_texture_free(p)
    return out


def save_png(path: str, packed: np.ndarray) -> None:
    """(h, w) uint32 0x00RRGGBB frame -> RGB PNG."""
    p = np.ascontiguousarray(packed, np.uint32)
    rc = lib().rtxh_image_save_png(path.encode(), p.ctypes.data, p.shape[1], p.shape[0])
    if rc:
        raise ValueError(f"rtxh_image_save_png({path!r}) failed with status {rc}")


def load_texture(path: str, mipmap_mode: bool = True) -> sio.Texture:
    """Texture::load (Texture.cpp:30-129): decode, sRGB -> linear, box-filter mips when both sides are powers of two."""
    p = C.POINTER(C.c_float)(); cnt = C.c_int64(); desc = RtxTextureDesc()
    rc = lib().rtxh_texture_load(path.encode(), 1 if mipmap_mode else 0, C.byref(p), C.byref(cnt), C.byref(desc))
    if rc:
        raise ValueError(f"rtxh_texture_load({path!r}) failed with status {rc}")
    texels = np.ctypeslib.as_array(p, (cnt.value, 3)).copy()
    lib().rtxh_texture_free(p)
    d = np.zeros(1, sio.TEXTURE_DESC)
    C.memmove(d.ctypes.data, C.byref(desc), C.sizeof(desc))
    return sio.Texture(d, texels)


_SRGB_LUT = None


def srgb8_to_linear(img_u8: np.ndarray) -> np.ndarray:
    """Texture::load's decode (Texture.cpp:13-20,64-72): byte * 0.00392156862f, then Math::gamma_to_linear
    (Math.h:78-88) with the host libm's powf — evaluated once per byte value into a 256-entry table."""
    global _SRGB_LUT
    if _SRGB_LUT is None:
        libm = C.CDLL("libm.so.6")
        libm.powf.restype = C.c_float; libm.powf.argtypes = [C.c_float, C.c_float]
        lut = np.zeros(256, np.float32)
        for b in range(256):
            x = np.float32(b) * np.float32(0.00392156862)
            if x <= 0: v = np.float32(0.0)
            elif x >= 1: v = np.float32(1.0)
            elif x < np.float32(0.04045): v = x / np.float32(12.92)
            else: v = np.float32(libm.powf(float((x + np.float32(0.055)) / np.float32(1.055)), 2.4))
            lut[b] = v
        _SRGB_LUT = lut
    return _SRGB_LUT[img_u8]


def synthetic_sky(n: int = 64) -> np.ndarray:
    """Seeded stand-in for Data/Sky_Probes/rnl_probe.float (absent from the reference mount);
    identical to the probe the golden vectors were rendered with (oracle/ref_harness/make_goldens.py)."""
    y, x = np.mgrid[0:n, 0:n]
    sky = np.zeros((n, n, 3), np.float32)
    sky[..., 0] = 0.5 + 0.5 * x / n
    sky[..., 1] = 0.6 + 0.2 * (((x // 8) + (y // 8)) & 1)
    sky[..., 2] = 0.5 + 0.5 * y / n
    return sky


def procedural_texture_images(seed: int) -> List[np.ndarray]:
    """The cfg3 stand-in's four power-of-two textures as 8-bit sRGB images (h, w, 3) — the form an asset file has."""
    rng = np.random.RandomState(seed & 0x7fffffff)

    def noise(n, octaves=4):
        out = np.zeros((n, n), np.float32)
        for o in range(octaves):
            k = 2 ** (o + 2)
            g = rng.rand(k, k).astype(np.float32)
            out += np.kron(g, np.ones((n // k, n // k), np.float32)) / (2 ** o)
        return out / out.max()

    texs = []
    n = 256   # floor tiles
    y, x = np.mgrid[0:n, 0:n]
    tile = (((x // 32) + (y // 32)) & 1).astype(np.float32)
    grout = ((x % 32 < 2) | (y % 32 < 2)).astype(np.float32)
    base = 0.55 + 0.25 * tile - 0.3 * grout + 0.1 * noise(n)
    texs.append(np.stack([base, base * 0.95, base * 0.85], -1))
    n = 512   # bricks
    y, x = np.mgrid[0:n, 0:n]
    row = y // 32
    xs = (x + (row & 1) * 32) % 64
    mortar = ((xs < 3) | (y % 32 < 3)).astype(np.float32)
    nb = noise(n)
    texs.append(np.stack([0.62 - 0.35 * mortar + 0.15 * nb, 0.34 - 0.1 * mortar + 0.1 * nb, 0.27 - 0.05 * mortar + 0.08 * nb], -1))
    n = 256   # stone
    s = 0.45 + 0.4 * noise(n, 5)
    texs.append(np.stack([s, s * 0.97, s * 0.9], -1))
    n = 256   # fabric stripes
    y, x = np.mgrid[0:n, 0:n]
    f = 0.6 + 0.3 * np.sin(x * (2 * np.pi / 16)).astype(np.float32) + 0.08 * noise(n)
    texs.append(np.stack([f, f, f], -1))
    return [np.clip(np.rint(np.clip(t, 0, 1) * 255.0), 0, 255).astype(np.uint8) for t in texs]


def _procedural_textures(seed: int) -> List[sio.Texture]:
    return [texture_with_mips(srgb8_to_linear(img)) for img in procedural_texture_images(seed)]


def make_config(width, height, bounces, mip_filter=1, texture_mode=2, stack_size=64, traversal=1, max_aniso=8.0, heatmap=0) -> np.ndarray:
    cfg = np.zeros(1, sio.CONFIG)
    cfg["width"] = width; cfg["height"] = height; cfg["bounces"] = bounces; cfg["stack_size"] = stack_size
    cfg["traversal_strategy"] = traversal; cfg["texture_mode"] = texture_mode; cfg["mip_filter"] = mip_filter
    cfg["max_anisotropy"] = max_aniso; cfg["heatmap"] = heatmap
    return cfg


ATRIUM_CAMERA = ((24.0, 5.5, 1.2), ((0.0, 1.0, 0.0), -1.45))     # position, (axis, angle)
ATRIUM_POINT = ((30.0, 26.0, 20.0), (-6.0, 9.0, 0.5))            # colour, position
ATRIUM_SPOT = ((40.0, 40.0, 48.0), (20.0, 14.0, -2.0), (-0.8, -0.55, 0.25), 50.0, 70.0)   # colour, position, direction, inner, outer (degrees)
ATRIUM_DIR = ((0.9, 0.9, 0.9), (0.1, -1.0, 0.1))                 # Scene.cpp:125


def atrium_mesh(seed: int = 0x5EED0003, detail: int = 1):
    """(positions (n,3,3), normals (n,3,3), texcoords (n,3,2) [v already flipped], material ids (n,), material count)."""
    mesh = RtxhMesh()
    assert lib().rtxh_atrium_generate(seed, detail, C.byref(mesh)) == 0
    n = mesh.triangle_count
    pos = np.ctypeslib.as_array(mesh.positions, (n, 3, 3)).copy()
    nrm = np.ctypeslib.as_array(mesh.normals, (n, 3, 3)).copy()
    uv = np.ctypeslib.as_array(mesh.texcoords, (n, 3, 2)).copy()
    mid = np.ctypeslib.as_array(mesh.material_ids, (n,)).copy()
    nmat = mesh.material_count
    lib().rtxh_mesh_free(C.byref(mesh))
    return pos, nrm, uv, mid, nmat


def atrium_materials(nmat: int) -> np.ndarray:
    """25 mesh-local materials mimicking sponza.mtl (Kd ~0.47, a few with Ks / Kt), texture ids into procedural_texture_images."""
    m = np.zeros(nmat, sio.MATERIAL)
    m["texture_id"] = -1; m["index_of_refraction"] = 1.0
    m["diffuse"] = 0.4704
    kd = {0: (0.75, 0.75, 0.75), 1: (0.8, 0.8, 0.8), 2: (0.7, 0.68, 0.6), 3: (0.8, 0.78, 0.74), 4: (0.6, 0.58, 0.5), 5: (0.75, 0.73, 0.7), 6: (0.5, 0.47, 0.4)}
    for k, v in kd.items():
        m["diffuse"][k] = v
    for k, v in {0: 0, 1: 1, 2: 1, 3: 2, 4: 2, 5: 2, 6: 2}.items():
        m["texture_id"][k] = v
    m["reflection"][0] = (0.15, 0.15, 0.15)                       # polished floor
    curtain = [(0.7, 0.1, 0.1), (0.1, 0.5, 0.15), (0.1, 0.15, 0.7), (0.7, 0.6, 0.1), (0.6, 0.1, 0.6), (0.1, 0.6, 0.6)]
    for i, c in enumerate(curtain):
        m["diffuse"][7 + i] = c; m["texture_id"][7 + i] = 3
    # vases: glass, metal, tinted glass, dark metal
    m["diffuse"][13] = (0.05, 0.05, 0.05); m["reflection"][13] = (0.25, 0.25, 0.25); m["transmittance"][13] = (0.95, 0.95, 0.95); m["index_of_refraction"][13] = 1.5
    m["diffuse"][14] = (0.3, 0.25, 0.1); m["reflection"][14] = (0.8, 0.7, 0.4)
    m["diffuse"][15] = (0.05, 0.1, 0.05); m["reflection"][15] = (0.2, 0.2, 0.2); m["transmittance"][15] = (0.6, 0.9, 0.7); m["index_of_refraction"][15] = 1.33
    m["diffuse"][16] = (0.1, 0.1, 0.12); m["reflection"][16] = (0.6, 0.6, 0.65)
    for i in range(4):                                               # statues: bronze-ish
        m["diffuse"][17 + i] = (0.45 - 0.05 * i, 0.3, 0.15 + 0.04 * i); m["reflection"][17 + i] = (0.12, 0.1, 0.06)
    m["diffuse"][21] = (0.35, 0.3, 0.25); m["diffuse"][22] = (0.6, 0.6, 0.6); m["diffuse"][23] = (0.85, 0.85, 0.8); m["diffuse"][24] = (0.5, 0.5, 0.5)
    return m


def atrium_scene(width: int = 1920, height: int = 1080, bounces: int = 3, detail: int = 1, seed: int = 0x5EED0003,
                 mip_filter: int = 1, bins: int = 32, accel: str = "sbvh") -> sio.Scene:
    """BASELINE.json configs[2]: Sponza-class (255 296 triangles at detail 1) stand-in, 3 lights,
    reflect/refract depth 3, anisotropic mip filter (the shipped default, Config.h:53).
    accel: "sbvh" = the reference's default builder restated (MESH_ACCELERATOR_SBVH, Config.h:35), "bvh" = its
    non-spatial builder, "binned" = this repo's own binned-SAH builder."""
    assert accel in ("sbvh", "bvh", "binned"), accel
    pos, nrm, uv, mid, nmat = atrium_mesh(seed, detail)
    sc = sio.Scene()
    sc.config = make_config(width, height, bounces, mip_filter=mip_filter)
    sc.textures = _procedural_textures(seed)
    # material table: 0 = MaterialBuffer default (Material.h:52-60), then the mesh's materials
    mats = np.zeros(1 + nmat, sio.MATERIAL)
    mats["texture_id"] = -1; mats["index_of_refraction"] = 1.0
    mats[1:] = atrium_materials(nmat)
    sc.materials = mats
    sc.blas = [build_blas(pos, nrm, uv, mid, material_offset=1, bins=bins, reference_sbvh=accel == "sbvh", reference_bvh=accel == "bvh")]
    root = sc.blas[0].nodes[0]
    inst, mn, mx = instance_update((0, 0, 0), (0, 0, 0, 1), root["aabb_min"], root["aabb_max"], 0)
    sc.instances = inst
    tl = Tlas(1)
    sc.tlas_nodes, sc.tlas_indices = tl.build(np.zeros((1, 3), np.float32), np.concatenate([mn, mx])[None])
    sc.sky = synthetic_sky()

    def normalize(v):                                                # Vector3::normalize, Vector3.h:24-31
        v = np.asarray(v, np.float32)
        inv = np.float32(1.0) / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2], dtype=np.float32)
        return v * inv
    deg2rad = lambda a: np.float32(a) * PI * np.float32(0.00555555555)   # DEG_TO_RAD, Util.h:14
    sc.dir_lights = np.zeros(1, sio.DIR_LIGHT); sc.dir_lights["colour"] = ATRIUM_DIR[0]; sc.dir_lights["negative_direction"] = -normalize(ATRIUM_DIR[1])
    sc.point_lights = np.zeros(1, sio.POINT_LIGHT); sc.point_lights["colour"] = ATRIUM_POINT[0]; sc.point_lights["position"] = ATRIUM_POINT[1]
    sc.spot_lights = np.zeros(1, sio.SPOT_LIGHT); sc.spot_lights["colour"] = ATRIUM_SPOT[0]; sc.spot_lights["position"] = ATRIUM_SPOT[1]
    sc.spot_lights["negative_direction"] = -normalize(ATRIUM_SPOT[2])
    sc.spot_lights["inner_cutoff"] = np.cos(deg2rad(np.float32(0.5) * np.float32(ATRIUM_SPOT[3])), dtype=np.float32)      # SpotLight.h:13-14
    sc.spot_lights["outer_cutoff"] = np.cos(deg2rad(np.float32(0.5) * np.float32(ATRIUM_SPOT[4])), dtype=np.float32)
    fov = float(deg2rad(110.0))                                                                                              # Scene.cpp:75
    sc.camera = camera_basis(width, height, fov, ATRIUM_CAMERA[0], axis_angle(*ATRIUM_CAMERA[1]))
    return sc
