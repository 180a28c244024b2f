"""ctypes binding of librtx_hip.so (the C ABI declared in include/rtx.h).

This is plumbing for tests and bench.py; the product is the shared library.  There is no CPU
fallback: if the HIP library is missing or no GPU is present, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np

from . import scene_io as sio
from .ctypes_structs import RtxConfig, RtxFrame, RtxStats, RtxWork, RtxTextureDesc, RtxAovBuffers, RtxRay, RtxQueryFilter, AOV_CHANNELS, RTX_AOV_ALL, fill_frame

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "..", "csrc", "librtx_hip.so")

EXPORTS = ["rtx_abi_version", "rtx_create", "rtx_destroy", "rtx_last_error", "rtx_upload_blas", "rtx_upload_materials",
           "rtx_upload_texture", "rtx_upload_sky", "rtx_set_frame", "rtx_render_tiles", "rtx_synchronize", "rtx_get_stats",
           "rtx_read_framebuffer", "rtx_framebuffer_device_ptrs", "rtx_last_kernel_times", "rtx_enable_kernel_timing",
           "rtx_bind_framebuffer", "rtx_set_stream", "rtx_present", "rtx_debug_libm", "rtx_debug_texture_sample", "rtx_debug_sky_sample", "rtx_debug_blas_wide", "rtx_debug_blas_wide_closest",
           "rtx_group_unique_id", "rtx_group_create", "rtx_group_render", "rtx_group_destroy", "rtx_group_attach", "rtx_group_create_local", "rtx_group_render_local",
           "rtx_group_layout", "rtx_group_slot_pixels", "rtx_debug_group_loopback", "rtx_debug_trace_rays", "rtx_debug_occluded", "rtx_debug_light_plot",
           "rtx_set_views", "rtx_render_views", "rtx_read_views", "rtx_bind_view_framebuffer", "rtx_bind_aovs", "rtx_read_aovs",
           "rtx_set_rays", "rtx_bind_rays", "rtx_render_rays", "rtx_update_instances", "rtx_read_frame_state",
           "rtx_bind_blas_vertices", "rtx_refit_blas", "rtx_read_blas", "rtx_alloc_blas", "rtx_build_blas",
           "rtx_query_closest", "rtx_query_occluded", "rtx_debug_query_order", "rtx_debug_read_layouts",
           "rtx_alloc_texture", "rtx_update_texture", "rtx_read_texture", "rtx_update_sky",
           "rtx_alloc_blas_topology", "rtx_set_blas_topology", "rtx_blas_vertex_normals", "rtx_query_nearest", "rtx_query_hits", "rtx_query_sweep",
           "rtx_debug_grids", "rtx_set_object_masks", "rtx_update_object_masks", "rtx_read_object_masks",
           "rtx_query_nearest_filtered", "rtx_query_hits_filtered", "rtx_query_sweep_filtered",
           "rtx_blas_pseudonormals", "rtx_read_blas_pseudonormals", "rtx_query_signed_distance",
           "rtx_query_overlap", "rtx_query_overlap_filtered", "rtx_query_sweep_box", "rtx_query_sweep_box_filtered",
           "rtx_query_overlap_capsule", "rtx_query_overlap_capsule_filtered"]
# newer than the A/B variants tools/ab.py may load (RTX_HIP_LIB = a library built from an older commit): bound when the library has them,
# otherwise a call raises AttributeError (undefined symbol)
VIEW_EXPORTS = ("rtx_set_views", "rtx_render_views", "rtx_read_views", "rtx_bind_view_framebuffer")
AOV_EXPORTS = ("rtx_bind_aovs", "rtx_read_aovs")
RAY_EXPORTS = ("rtx_set_rays", "rtx_bind_rays", "rtx_render_rays")
UPDATE_EXPORTS = ("rtx_update_instances", "rtx_read_frame_state")
REFIT_EXPORTS = ("rtx_bind_blas_vertices", "rtx_refit_blas", "rtx_read_blas")
BUILD_EXPORTS = ("rtx_alloc_blas", "rtx_build_blas")
QUERY_EXPORTS = ("rtx_query_closest", "rtx_query_occluded")
QUERY_SORT_EXPORTS = ("rtx_debug_query_order",)
LAYOUT_EXPORTS = ("rtx_debug_read_layouts",)
TEXTURE_EXPORTS = ("rtx_alloc_texture", "rtx_update_texture", "rtx_read_texture", "rtx_update_sky")
NORMALS_EXPORTS = ("rtx_alloc_blas_topology", "rtx_set_blas_topology", "rtx_blas_vertex_normals")
NEAREST_EXPORTS = ("rtx_query_nearest",)
SIGNED_EXPORTS = ("rtx_blas_pseudonormals", "rtx_read_blas_pseudonormals", "rtx_query_signed_distance")
HITS_EXPORTS = ("rtx_query_hits",)
SWEEP_EXPORTS = ("rtx_query_sweep",)
GRID_EXPORTS = ("rtx_debug_grids",)
MASK_EXPORTS = ("rtx_set_object_masks", "rtx_update_object_masks", "rtx_read_object_masks",
                "rtx_query_nearest_filtered", "rtx_query_hits_filtered", "rtx_query_sweep_filtered")
OVERLAP_EXPORTS = ("rtx_query_overlap", "rtx_query_overlap_filtered")
SWEEP_BOX_EXPORTS = ("rtx_query_sweep_box", "rtx_query_sweep_box_filtered")
OVERLAP_CAPSULE_EXPORTS = ("rtx_query_overlap_capsule", "rtx_query_overlap_capsule_filtered")
OPTIONAL_EXPORTS = (OVERLAP_CAPSULE_EXPORTS + SWEEP_BOX_EXPORTS + OVERLAP_EXPORTS + VIEW_EXPORTS + AOV_EXPORTS + RAY_EXPORTS + UPDATE_EXPORTS + REFIT_EXPORTS + QUERY_EXPORTS + QUERY_SORT_EXPORTS + LAYOUT_EXPORTS
                    + TEXTURE_EXPORTS + NORMALS_EXPORTS + NEAREST_EXPORTS + HITS_EXPORTS + SWEEP_EXPORTS + GRID_EXPORTS + MASK_EXPORTS + SIGNED_EXPORTS)
RTX_QUERY_MAX_HITS = 8
# texel formats of rtx_update_texture (include/rtx.h RTX_TEXELS_*)
RTX_TEXELS_RGB_F32 = 0
RTX_TEXELS_RGBA8_SRGB = 1
RTX_UPDATE_MAX_INSTANCES = 65536
RTX_ERR_STATE = 5

RTX_RENDER_COUNT_WORK = 1
RTX_RENDER_SIMPLE_TRACE = 2
RTX_RENDER_CULL_DEAD_SHADOW_RAYS = 4
RTX_RENDER_SERIAL = 8
RTX_RENDER_LANE_TRACE = 16
RTX_RENDER_PACKET_STATS = 32
RTX_RENDER_PACKET_CLOSEST = 64
RTX_RENDER_AOV = 128
RTX_MAX_VIEWS = 4096
# ray queries (include/rtx.h RTX_QUERY_*): the RTX_AOV_* bits of the same meaning, no albedo
RTX_QUERY_DISTANCE = 1
RTX_QUERY_POSITION = 2
RTX_QUERY_NORMAL = 4
RTX_QUERY_UV = 16
RTX_QUERY_MATERIAL_ID = 32
RTX_QUERY_OBJECT_ID = 64
RTX_QUERY_TRIANGLE_ID = 128
RTX_QUERY_ALL = 247
RTX_QUERY_CHUNK_RAYS = 1 << 20
RTX_OVERLAP_OBJECTS = 512   # bits of rtx_query_overlap's flags: the distinct objects; 0 / 1 per row
RTX_OVERLAP_ANY = 1024
RTX_QUERY_SORT = 256        # a bit of the query calls' flags: sort the rays of every round into coherent packets on the device
# name -> (bit, numpy dtype, components per ray), in rtx_query_buffers order
QUERY_CHANNELS = {"distance": (RTX_QUERY_DISTANCE, np.float32, 1), "position": (RTX_QUERY_POSITION, np.float32, 3),
                  "normal": (RTX_QUERY_NORMAL, np.float32, 3), "uv": (RTX_QUERY_UV, np.float32, 2),
                  "material_id": (RTX_QUERY_MATERIAL_ID, np.int32, 1), "object_id": (RTX_QUERY_OBJECT_ID, np.int32, 1),
                  "triangle_id": (RTX_QUERY_TRIANGLE_ID, np.int32, 1)}


class RtxQueryBuffers(C.Structure):
    """rtx_query_buffers: one device pointer per channel, None = not written."""
    _fields_ = [(name, C.c_void_p) for name in QUERY_CHANNELS]


ERRORS = {1: "RTX_ERR_INVALID_ARG", 2: "RTX_ERR_NO_DEVICE", 3: "RTX_ERR_HIP", 4: "RTX_ERR_LIMIT", 5: "RTX_ERR_STATE", 6: "RTX_ERR_OOM"}

_lib = None


class RtxError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        super().__init__(f"{where}: {ERRORS.get(code, code)} {detail}")


def load_library(path: Optional[str] = None):
    """Load librtx_hip.so; raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.abspath(path or os.environ.get("RTX_HIP_LIB") or LIB_PATH)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: the HIP extension has not been built (python -c 'import __graft_entry__ as g; g.build()')")
    lib = C.CDLL(path)
    vp, i32, u32, f = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    lib.rtx_abi_version.restype = C.c_int
    lib.rtx_create.argtypes = [C.POINTER(RtxConfig), C.POINTER(vp)]
    lib.rtx_destroy.argtypes = [vp]
    lib.rtx_last_error.argtypes = [vp]; lib.rtx_last_error.restype = C.c_char_p
    lib.rtx_upload_blas.argtypes = [vp, i32, vp, i32, vp, vp, i32, i32]
    lib.rtx_upload_materials.argtypes = [vp, vp, i32]
    lib.rtx_upload_texture.argtypes = [vp, i32, C.POINTER(RtxTextureDesc), vp, C.c_int64]
    lib.rtx_upload_sky.argtypes = [vp, vp, i32]
    lib.rtx_set_frame.argtypes = [vp, C.POINTER(RtxFrame)]
    lib.rtx_render_tiles.argtypes = [vp, i32, i32, i32, u32]
    lib.rtx_synchronize.argtypes = [vp]
    lib.rtx_get_stats.argtypes = [vp, C.POINTER(RtxStats), C.POINTER(RtxWork)]
    lib.rtx_read_framebuffer.argtypes = [vp, vp, vp]
    lib.rtx_framebuffer_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.rtx_last_kernel_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(f), i32, C.POINTER(i32)]
    lib.rtx_enable_kernel_timing.argtypes = [vp, i32]
    lib.rtx_bind_framebuffer.argtypes = [vp, vp, vp]
    lib.rtx_set_stream.argtypes = [vp, vp]
    lib.rtx_present.argtypes = [vp, i32, vp, C.POINTER(vp)]
    lib.rtx_debug_libm.argtypes = [vp, i32, vp, vp, vp, i32]
    lib.rtx_debug_texture_sample.argtypes = [vp, i32, vp, vp, i32]
    lib.rtx_debug_sky_sample.argtypes = [vp, vp, vp, i32]
    lib.rtx_debug_blas_wide.argtypes = [vp, i32, vp]
    lib.rtx_debug_blas_wide_closest.argtypes = [vp, i32, vp]
    lib.rtx_group_unique_id.argtypes = [vp]
    lib.rtx_group_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    lib.rtx_group_attach.argtypes = [vp, vp, C.POINTER(vp)]
    lib.rtx_group_render.argtypes = [vp, u32]
    lib.rtx_group_destroy.argtypes = [vp]
    lib.rtx_group_create_local.argtypes = [C.POINTER(vp), i32, C.POINTER(vp)]
    lib.rtx_group_render_local.argtypes = [C.POINTER(vp), i32, u32]
    lib.rtx_debug_group_loopback.argtypes = [vp, i32, u32]
    lib.rtx_group_layout.argtypes = [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.rtx_group_slot_pixels.argtypes = [i32, i32, i32, i32, vp, C.c_int64]
    lib.rtx_debug_trace_rays.argtypes = [vp, vp, i32, vp, u32]
    lib.rtx_debug_occluded.argtypes = [vp, vp, i32, vp, u32]
    lib.rtx_debug_light_plot.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32]
    if hasattr(lib, "rtx_set_views"):
        lib.rtx_set_views.argtypes = [vp, vp, i32]
        lib.rtx_render_views.argtypes = [vp, i32, i32, u32]
        lib.rtx_read_views.argtypes = [vp, i32, i32, vp, vp]
        lib.rtx_bind_view_framebuffer.argtypes = [vp, vp, vp, i32]
    if hasattr(lib, "rtx_bind_aovs"):
        lib.rtx_bind_aovs.argtypes = [vp, u32, C.POINTER(RtxAovBuffers), C.c_int64]
        lib.rtx_read_aovs.argtypes = [vp, i32, i32, C.POINTER(RtxAovBuffers)]
    if hasattr(lib, "rtx_set_rays"):
        lib.rtx_set_rays.argtypes = [vp, vp, i32]
        lib.rtx_bind_rays.argtypes = [vp, vp, i32]
        lib.rtx_render_rays.argtypes = [vp, i32, i32, u32]
    if hasattr(lib, "rtx_update_instances"):
        lib.rtx_update_instances.argtypes = [vp, vp, vp, i32]
        lib.rtx_read_frame_state.argtypes = [vp, vp, vp, C.POINTER(i32), vp]
    if hasattr(lib, "rtx_refit_blas"):
        lib.rtx_bind_blas_vertices.argtypes = [vp, i32, vp, i32]
        lib.rtx_refit_blas.argtypes = [vp, i32, vp, vp, i32]
        lib.rtx_read_blas.argtypes = [vp, i32, vp, vp, vp]
    if hasattr(lib, "rtx_build_blas"):
        lib.rtx_alloc_blas.argtypes = [vp, i32, i32, i32, vp, i32]
        lib.rtx_build_blas.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    if hasattr(lib, "rtx_query_closest"):
        lib.rtx_query_closest.argtypes = [vp, vp, C.c_int64, u32, C.POINTER(RtxQueryBuffers), u32]
        lib.rtx_query_occluded.argtypes = [vp, vp, C.c_int64, vp, u32]
    if hasattr(lib, "rtx_query_nearest"):
        lib.rtx_query_nearest.argtypes = [vp, vp, C.c_int64, u32, C.POINTER(RtxQueryBuffers), u32]
    if hasattr(lib, "rtx_query_sweep"):
        lib.rtx_query_sweep.argtypes = [vp, vp, C.c_int64, u32, C.POINTER(RtxQueryBuffers), u32]
    if hasattr(lib, "rtx_query_hits"):
        lib.rtx_query_hits.argtypes = [vp, vp, C.c_int64, i32, u32, C.POINTER(RtxQueryBuffers), vp, u32]
    if hasattr(lib, "rtx_set_object_masks"):
        lib.rtx_set_object_masks.argtypes = [vp, vp, i32]
        lib.rtx_update_object_masks.argtypes = [vp, vp, i32]
        lib.rtx_read_object_masks.argtypes = [vp, vp, i32, C.POINTER(i32)]
        lib.rtx_query_nearest_filtered.argtypes = [vp, vp, C.c_int64, u32, C.POINTER(RtxQueryBuffers), u32, C.POINTER(RtxQueryFilter)]
        lib.rtx_query_sweep_filtered.argtypes = [vp, vp, C.c_int64, u32, C.POINTER(RtxQueryBuffers), u32, C.POINTER(RtxQueryFilter)]
        lib.rtx_query_hits_filtered.argtypes = [vp, vp, C.c_int64, i32, u32, C.POINTER(RtxQueryBuffers), vp, u32, C.POINTER(RtxQueryFilter)]
    if hasattr(lib, "rtx_debug_query_order"):
        lib.rtx_debug_query_order.argtypes = [vp, vp, i32, C.c_int64, vp]
    if hasattr(lib, "rtx_debug_read_layouts"):
        lib.rtx_debug_read_layouts.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "rtx_debug_grids"):
        lib.rtx_debug_grids.argtypes = [vp, vp]
    if hasattr(lib, "rtx_update_texture"):
        lib.rtx_alloc_texture.argtypes = [vp, i32, i32, i32, i32]
        lib.rtx_update_texture.argtypes = [vp, i32, vp, i32]
        lib.rtx_read_texture.argtypes = [vp, i32, C.POINTER(RtxTextureDesc), vp, C.c_int64]
        lib.rtx_update_sky.argtypes = [vp, vp, i32]
    if hasattr(lib, "rtx_blas_vertex_normals"):
        lib.rtx_alloc_blas_topology.argtypes = [vp, i32, i32, i32]
        lib.rtx_set_blas_topology.argtypes = [vp, i32, vp]
        lib.rtx_blas_vertex_normals.argtypes = [vp, i32, vp, vp]
    if hasattr(lib, "rtx_query_signed_distance"):
        lib.rtx_blas_pseudonormals.argtypes = [vp, i32, vp]
        lib.rtx_read_blas_pseudonormals.argtypes = [vp, i32, vp, vp]
        lib.rtx_query_signed_distance.argtypes = [vp, vp, C.c_int64, u32, C.POINTER(RtxQueryBuffers), vp, vp, u32, C.POINTER(RtxQueryFilter)]
    if hasattr(lib, "rtx_query_overlap"):
        lib.rtx_query_overlap.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp, u32]
        lib.rtx_query_overlap_filtered.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp, u32, C.POINTER(RtxQueryFilter)]
    if hasattr(lib, "rtx_query_overlap_capsule"):
        lib.rtx_query_overlap_capsule.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp, u32]
        lib.rtx_query_overlap_capsule_filtered.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp, u32, C.POINTER(RtxQueryFilter)]
    if hasattr(lib, "rtx_query_sweep_box"):
        lib.rtx_query_sweep_box.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, u32]
        lib.rtx_query_sweep_box_filtered.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp, u32, C.POINTER(RtxQueryFilter)]
    for name in EXPORTS:
        if name in OPTIONAL_EXPORTS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        if name not in ("rtx_last_error",):
            fn.restype = C.c_int
    _lib = lib
    return lib


def render_flags(count_work: bool = False, simple_trace: bool = False, cull_dead_shadow_rays: bool = False, serial: bool = False,
                 lane_trace: bool = False, packet_stats: bool = False, packet_closest: bool = False, aov: bool = False) -> int:
    """The RTX_RENDER_* bits of the keyword flags Renderer.render / render_views take."""
    return ((RTX_RENDER_COUNT_WORK if count_work else 0) | (RTX_RENDER_SIMPLE_TRACE if simple_trace else 0)
            | (RTX_RENDER_CULL_DEAD_SHADOW_RAYS if cull_dead_shadow_rays else 0) | (RTX_RENDER_SERIAL if serial else 0)
            | (RTX_RENDER_LANE_TRACE if lane_trace else 0) | (RTX_RENDER_PACKET_STATS if packet_stats else 0)
            | (RTX_RENDER_PACKET_CLOSEST if packet_closest else 0) | (RTX_RENDER_AOV if aov else 0))


def aov_names(channels) -> tuple:
    """AOV channel names (keys of ctypes_structs.AOV_CHANNELS, in that order) of a RTX_AOV_* mask, one name or an iterable of names.
    Raises before anything reaches the library."""
    if isinstance(channels, (int, np.integer)) and not isinstance(channels, bool):
        if not 0 <= int(channels) <= RTX_AOV_ALL:
            raise ValueError(f"AOV channel mask {channels} has bits outside RTX_AOV_ALL")
        return tuple(n for n, (bit, _, _) in AOV_CHANNELS.items() if int(channels) & bit)
    if isinstance(channels, str):
        channels = (channels,)
    names = set()
    for n in channels:
        if not isinstance(n, str):
            raise TypeError(f"AOV channels are names ({', '.join(AOV_CHANNELS)}), not {type(n).__name__}")
        if n not in AOV_CHANNELS:
            raise ValueError(f"unknown AOV channel {n!r} (known: {', '.join(AOV_CHANNELS)})")
        names.add(n)
    return tuple(n for n in AOV_CHANNELS if n in names)


def aov_mask(channels) -> int:
    """RTX_AOV_* bits of a mask, one channel name or an iterable of names."""
    return sum(AOV_CHANNELS[n][0] for n in aov_names(channels))


def aov_shape(name: str, views: Optional[int], height: int, width: int) -> tuple:
    """Shape of channel `name` for `views` views ((H, W[, k]) when views is None)."""
    k = AOV_CHANNELS[name][2]
    return ((views,) if views is not None else ()) + (height, width) + ((k,) if k > 1 else ())


def query_names(channels) -> tuple:
    """Ray-query channel names (keys of QUERY_CHANNELS, in that order) of a RTX_QUERY_* mask, one name or an iterable of names; at least
    one.  Raises before anything reaches the library."""
    if isinstance(channels, (int, np.integer)) and not isinstance(channels, bool):
        if int(channels) & ~RTX_QUERY_ALL or int(channels) < 0:
            raise ValueError(f"query channel mask {channels} has bits outside RTX_QUERY_ALL")
        names = tuple(n for n, (bit, _, _) in QUERY_CHANNELS.items() if int(channels) & bit)
    else:
        if isinstance(channels, str):
            channels = (channels,)
        want = set()
        for n in channels:
            if not isinstance(n, str):
                raise TypeError(f"query channels are names ({', '.join(QUERY_CHANNELS)}), not {type(n).__name__}")
            if n not in QUERY_CHANNELS:
                raise ValueError(f"unknown query channel {n!r} (known: {', '.join(QUERY_CHANNELS)})")
            want.add(n)
        names = tuple(n for n in QUERY_CHANNELS if n in want)
    if not names:
        raise ValueError("a query needs at least one channel")
    return names


def views_array(cameras) -> np.ndarray:
    """Cameras for rtx_set_views as a contiguous scene_io.CAMERA array of shape (V,): accepts that, or float32 (V, 12) rows of
    (position, rotated_top_left_corner, rotated_x_axis, rotated_y_axis).  Raises before anything reaches the library."""
    if not isinstance(cameras, np.ndarray):
        raise TypeError(f"cameras must be a numpy array (scene_io.CAMERA (V,) or float32 (V, 12)), not {type(cameras).__name__}")
    if cameras.dtype == sio.CAMERA:
        if cameras.ndim != 1:
            raise ValueError(f"a scene_io.CAMERA array of views must have shape (V,), not {cameras.shape}")
        cams = np.ascontiguousarray(cameras)
    elif cameras.dtype == np.float32:
        if cameras.ndim != 2 or cameras.shape[1] != 12:
            raise ValueError(f"float32 cameras must have shape (V, 12), not {cameras.shape}")
        cams = np.ascontiguousarray(cameras).view(sio.CAMERA).reshape(-1)
    else:
        raise TypeError(f"cameras must be scene_io.CAMERA or float32, not {cameras.dtype}")
    if not 1 <= cams.shape[0] <= RTX_MAX_VIEWS:
        raise ValueError(f"1 .. {RTX_MAX_VIEWS} views, not {cams.shape[0]}")
    return cams


RAY_FLOATS = C.sizeof(RtxRay) // 4          # 18: origin, direction, dO_dx, dO_dy, dD_dx, dD_dy


def rays_array(rays, width: int, height: int) -> np.ndarray:
    """Rays for rtx_set_rays as a contiguous float32 (V, H, W, 18) array: accepts that or (H, W, 18).  Raises before anything reaches
    the library."""
    if not isinstance(rays, np.ndarray):
        raise TypeError(f"rays must be a numpy float32 array (V, H, W, {RAY_FLOATS}) or (H, W, {RAY_FLOATS}), not {type(rays).__name__}")
    if rays.dtype != np.float32:
        raise TypeError(f"rays must be float32, not {rays.dtype}")
    if rays.ndim == 3:
        rays = rays[None]
    if rays.ndim != 4:
        raise ValueError(f"rays must have shape (V, H, W, {RAY_FLOATS}) or (H, W, {RAY_FLOATS}), not {rays.shape}")
    if rays.shape[3] != RAY_FLOATS:
        raise ValueError(f"a ray is {RAY_FLOATS} floats (origin, direction, dO_dx, dO_dy, dD_dx, dD_dy), not {rays.shape[3]}")
    if rays.shape[1] != height or rays.shape[2] != width:
        raise ValueError(f"rays must be (V, {height}, {width}, {RAY_FLOATS}) for this context, not {rays.shape}")
    if not 1 <= rays.shape[0] <= RTX_MAX_VIEWS:
        raise ValueError(f"1 .. {RTX_MAX_VIEWS} ray views, not {rays.shape[0]}")
    return np.ascontiguousarray(rays)


def pinhole_rays(camera, width: int, height: int) -> np.ndarray:
    """(H, W, 18) float32: the primary rays of Raytracer::render_tile (Raytracer.cpp:30-59) for `camera` (one scene_io.CAMERA record, or 12
    floats: position, rotated_top_left_corner, rotated_x_axis, rotated_y_axis) in the oracle's and the kernels' operation order: unfused
    multiply and add, correctly rounded sqrt and divide, dot products as x*x + (y*y + z*z), zero origin differentials.  Rendering them with
    render_rays gives the bits of the camera's own frame."""
    f32 = np.float32
    cam = np.asarray(camera)
    if cam.dtype == sio.CAMERA:
        cam = np.ascontiguousarray(cam).reshape(-1)[:1].view(f32)
    cam = np.ascontiguousarray(cam, f32).reshape(-1)
    if cam.shape[0] != 12:
        raise ValueError(f"a camera is 12 floats (position, top-left corner, x axis, y axis), not {cam.shape[0]}")
    pos, tl, ax, ay = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    j, i = np.meshgrid(np.arange(height, dtype=f32), np.arange(width, dtype=f32), indexing="ij")
    i = i.reshape(-1, 1); j = j.reshape(-1, 1)
    d = ax * i + (ay * j + tl)                                               # vmadd_s(ax, is, vmadd_s(ay, js, tl))

    def dot(a, b):
        return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
    dd = dot(d, d)
    inv = f32(1.0) / np.sqrt(dd)
    denom = inv / dd
    axb = np.broadcast_to(ax, d.shape); ayb = np.broadcast_to(ay, d.shape)
    rays = np.zeros((d.shape[0], RAY_FLOATS), f32)
    rays[:, 0:3] = pos
    rays[:, 3:6] = d * inv[:, None]
    rays[:, 12:15] = (ax * dd[:, None] - d * dot(d, axb)[:, None]) * denom[:, None]
    rays[:, 15:18] = (ay * dd[:, None] - d * dot(d, ayb)[:, None]) * denom[:, None]
    return rays.reshape(height, width, RAY_FLOATS)


def rays_from_directions(origins, directions) -> np.ndarray:
    """(H, W, 18) float32 rays of per-pixel origins and directions, both (H, W, 3): the differentials are forward differences between
    neighbouring pixels (d/dx: column x + 1 minus column x, d/dy: row y + 1 minus row y); the last column / row uses the backward
    difference, a single column / row gets zero.  A convenience for camera models without analytic differentials (they only steer the
    texture level of detail); it is not parity with anything."""
    o = np.asarray(origins, np.float32); d = np.asarray(directions, np.float32)
    if o.ndim != 3 or o.shape[2] != 3 or o.shape != d.shape:
        raise ValueError(f"origins and directions must both be (H, W, 3), not {o.shape} and {d.shape}")

    def diff(a, axis):
        out = np.zeros_like(a)
        if a.shape[axis] > 1:
            f = np.diff(a, axis=axis)
            if axis == 1:
                out[:, :-1] = f; out[:, -1] = f[:, -1]
            else:
                out[:-1] = f; out[-1] = f[-1]
        return out
    return np.ascontiguousarray(np.concatenate([o, d, diff(o, 1), diff(o, 0), diff(d, 1), diff(d, 0)], axis=2), np.float32)


def grid_boxes(origin, cell, shape, device=None):
    """The query_overlap rows of a voxel grid: float32 (X*Y*Z, 10), voxel (x, y, z) at row x + X * (y + Y * z) — x fastest — with centre
    origin + (index + 0.5) * cell, half extents cell / 2 and the identity quaternion.  origin = the grid's minimum corner (3,), cell = the
    voxel size (a number or (3,)), shape = (X, Y, Z).  device=None: a numpy array; otherwise a torch tensor on that device, so that
    query_overlapped(grid_boxes(...)).view(Z, Y, X) is an occupancy grid."""
    o = np.asarray(origin, np.float64).reshape(-1)
    c = np.asarray(cell, np.float64).reshape(-1)
    if c.size == 1:
        c = np.repeat(c, 3)
    dims = tuple(int(v) for v in shape)
    if o.size != 3 or c.size != 3 or len(dims) != 3:
        raise ValueError("origin and cell must have 3 components (cell may be one number) and shape must be (X, Y, Z)")
    if min(dims) < 1 or not np.all(np.isfinite(o)) or not np.all(np.isfinite(c)) or np.any(c <= 0):
        raise ValueError(f"shape {dims} must be positive and origin / cell finite with cell > 0")
    X, Y, Z = dims
    rows = np.zeros((Z, Y, X, 10), np.float32)
    rows[..., 0] = (o[0] + (np.arange(X) + 0.5) * c[0])[None, None, :]
    rows[..., 1] = (o[1] + (np.arange(Y) + 0.5) * c[1])[None, :, None]
    rows[..., 2] = (o[2] + (np.arange(Z) + 0.5) * c[2])[:, None, None]
    rows[..., 3:6] = (0.5 * c).astype(np.float32)
    rows[..., 9] = 1.0
    rows = rows.reshape(-1, 10)
    if device is None:
        return rows
    import torch
    return torch.from_numpy(rows).to(device)


def capsule_rows(a, b, radius, device=None):
    """The query_overlap_capsule rows of capsules given by their end points: float32 (n, 7) of (p = a, d = b - a, r = radius).  a, b = (n, 3)
    (or (3,)), radius = a number or (n,); b == a makes a ball.  d is rounded once, from the float32 end points.  device=None: a numpy array;
    otherwise a torch tensor on that device."""
    pa = np.atleast_2d(np.asarray(a, np.float32))
    pb = np.atleast_2d(np.asarray(b, np.float32))
    if pa.ndim != 2 or pa.shape[1] != 3 or pa.shape != pb.shape:
        raise ValueError(f"a and b must both have shape (n, 3), not {pa.shape} and {pb.shape}")
    r = np.asarray(radius, np.float32).reshape(-1)
    if r.size not in (1, pa.shape[0]):
        raise ValueError(f"radius must be one number or have shape ({pa.shape[0]},), not {np.shape(radius)}")
    rows = np.zeros((pa.shape[0], 7), np.float32)
    rows[:, 0:3] = pa
    rows[:, 3:6] = pb - pa
    rows[:, 6] = r
    if device is None:
        return rows
    import torch
    return torch.from_numpy(rows).to(device)


def group_layout(width: int, height: int, world: int, rank: int):
    """(tiles_total, tiles_per_rank, own_tiles) of rank `rank` of `world` (rtx_group_layout: host function, no GPU needed).  The rank
    renders rtx_render_tiles(first_tile=rank, tile_stride=world, tile_count=own_tiles)."""
    lib = load_library()
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.rtx_group_layout(width, height, world, rank, C.byref(a), C.byref(b), C.byref(c))
    if rc:
        raise RtxError(rc, "rtx_group_layout")
    return a.value, b.value, c.value


def group_slot_pixels(width: int, height: int, world: int, rank: int) -> np.ndarray:
    """Raster pixel index of every slot of the rank's tile-major send buffer, -1 = padding (rtx_group_slot_pixels: the kernels' own index maths, on the host)."""
    lib = load_library()
    _, per_rank, _ = group_layout(width, height, world, rank)
    out = np.empty(per_rank * 1024, np.int64)
    rc = lib.rtx_group_slot_pixels(width, height, world, rank, out.ctypes.data, out.size)
    if rc:
        raise RtxError(rc, "rtx_group_slot_pixels")
    return out


class Renderer:
    """One rtx_ctx: uploads a Scene and renders tiles of it on one GPU."""

    def __init__(self, scene: sio.Scene, device: int = 0, upload: bool = True):
        self.lib = load_library()
        self.scene = scene
        cfg = RtxConfig()
        C.memmove(C.byref(cfg), scene.config.ctypes.data, C.sizeof(RtxConfig))
        cfg.device = device
        self.device = device
        self.ctx = C.c_void_p()
        rc = self.lib.rtx_create(C.byref(cfg), C.byref(self.ctx))
        if rc:
            self.ctx = None
            raise RtxError(rc, "rtx_create")
        self._keep: List[np.ndarray] = []
        self.ray_view_count = 0          # ray views in the context's own buffer (set_rays)
        self.frame_instance_count = 0    # instances of the frame last set (set_frame)
        self._rays_bound = None          # (device pointer, views) bound with bind_rays
        self._blas_shapes: List[Optional[tuple]] = []      # per uploaded BLAS id: (nodes, slots, material offset, source triangles) — read_blas sizes its arrays by it
        if upload:
            self.upload_scene(scene)
            self.set_frame(scene)

    def _chk(self, rc: int, where: str):
        if rc:
            raise RtxError(rc, where, (self.lib.rtx_last_error(self.ctx) or b"").decode())

    def close(self):
        if self.ctx and getattr(self, "group", None):
            self.group_destroy()
        if self.ctx:
            self.lib.rtx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # The plain uploads (include/rtx.h, "scene data that lives across frames").  Each may be called at any time, also after set_frame: it
    # waits for the queued work and takes effect at the next render or query call, with no set_frame in between.
    def upload_blas(self, blas_id: int, b: sio.Blas):
        """b under blas_id (new, or replacing what the id held: a vertex binding and what alloc_blas made of the id go with it)."""
        nodes = np.ascontiguousarray(b.nodes); hot = np.ascontiguousarray(b.tri_hot); cold = np.ascontiguousarray(b.tri_cold)
        self._chk(self.lib.rtx_upload_blas(self.ctx, int(blas_id), nodes.ctypes.data, len(nodes), hot.ctypes.data, cold.ctypes.data,
                                           len(hot), b.material_offset), "rtx_upload_blas")
        self._blas_shapes += [None] * (blas_id + 1 - len(self._blas_shapes))
        self._blas_shapes[blas_id] = (len(nodes), len(hot), b.material_offset, b.source_triangle_count)
        getattr(self, "_built_shapes", {}).pop(int(blas_id), None)      # no longer an alloc_blas id

    def upload_materials(self, materials):
        """The whole material table (scene_io.MATERIAL array), of any count >= 1."""
        mats = np.ascontiguousarray(materials)
        if mats.ndim != 1 or mats.dtype.itemsize != sio.MATERIAL.itemsize:
            raise ValueError(f"materials must be a 1-d array of scene_io.MATERIAL, not {mats.dtype} {mats.shape}")
        self._chk(self.lib.rtx_upload_materials(self.ctx, mats.ctypes.data, len(mats)), "rtx_upload_materials")

    def upload_texture(self, texture_id: int, t: sio.Texture):
        """t (descriptor and float texels, chain included) under texture_id."""
        desc = RtxTextureDesc()
        C.memmove(C.byref(desc), t.desc.ctypes.data, C.sizeof(RtxTextureDesc))
        tex = np.ascontiguousarray(t.texels, np.float32)
        self._chk(self.lib.rtx_upload_texture(self.ctx, int(texture_id), C.byref(desc), tex.ctypes.data, len(tex)), "rtx_upload_texture")

    def upload_sky(self, sky):
        """The sky probe, (S, S, 3) float32 of any size S."""
        sky = np.ascontiguousarray(sky, np.float32)
        self._chk(self.lib.rtx_upload_sky(self.ctx, sky.ctypes.data, sky.shape[0]), "rtx_upload_sky")

    def upload_scene(self, sc: sio.Scene):
        for i, b in enumerate(sc.blas):
            self.upload_blas(i, b)
        self.upload_materials(sc.materials)
        for i, t in enumerate(sc.textures):
            self.upload_texture(i, t)
        self.upload_sky(sc.sky)

    def set_frame(self, sc: sio.Scene):
        fr = RtxFrame()
        keep: List[np.ndarray] = []
        fill_frame(fr, sc, keep)
        self._chk(self.lib.rtx_set_frame(self.ctx, C.byref(fr)), "rtx_set_frame")
        self.frame_instance_count = len(sc.instances)      # what the context now holds (read_frame_state sizes its arrays by it)

    def render_async(self, first_tile: int = 0, tile_stride: int = 1, tile_count: Optional[int] = None, count_work: bool = False,
                     simple_trace: bool = False, cull_dead_shadow_rays: bool = False, serial: bool = False, lane_trace: bool = False,
                     packet_stats: bool = False, packet_closest: bool = False, aov: bool = False):
        if tile_count is None:
            tile_count = (self.scene.tile_count - first_tile + tile_stride - 1) // tile_stride
        flags = render_flags(count_work, simple_trace, cull_dead_shadow_rays, serial, lane_trace, packet_stats, packet_closest, aov)
        self._chk(self.lib.rtx_render_tiles(self.ctx, first_tile, tile_stride, tile_count, flags), "rtx_render_tiles")

    def synchronize(self):
        self._chk(self.lib.rtx_synchronize(self.ctx), "rtx_synchronize")

    def stats(self):
        st, wk = RtxStats(), RtxWork()
        self._chk(self.lib.rtx_get_stats(self.ctx, C.byref(st), C.byref(wk)), "rtx_get_stats")
        return st.as_dict(), wk.as_dict()

    def framebuffer(self):
        sc = self.scene
        rgb = np.zeros((sc.height, sc.width, 3), np.float32)
        packed = np.zeros((sc.height, sc.width), np.uint32)
        self._chk(self.lib.rtx_read_framebuffer(self.ctx, rgb.ctypes.data, packed.ctypes.data), "rtx_read_framebuffer")
        return rgb, packed

    def present(self, fxaa: bool = True) -> np.ndarray:
        """Window::draw_quad: the displayed image (gamma 1/2.2, optional FXAA) of the frame in the framebuffer, (h, w) 0x00RRGGBB."""
        out = np.zeros((self.scene.height, self.scene.width), np.uint32)
        self._chk(self.lib.rtx_present(self.ctx, 1 if fxaa else 0, out.ctypes.data, None), "rtx_present")
        return out

    def device_ptrs(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self.lib.rtx_framebuffer_device_ptrs(self.ctx, C.byref(a), C.byref(b)), "rtx_framebuffer_device_ptrs")
        return a.value, b.value

    def render(self, first_tile: int = 0, tile_stride: int = 1, tile_count: Optional[int] = None, count_work: bool = False,
               simple_trace: bool = False, cull_dead_shadow_rays: bool = False, serial: bool = False, lane_trace: bool = False,
               packet_stats: bool = False, packet_closest: bool = False) -> Dict:
        self.render_async(first_tile, tile_stride, tile_count, count_work, simple_trace, cull_dead_shadow_rays, serial, lane_trace, packet_stats, packet_closest)
        stats, work = self.stats()
        rgb, packed = self.framebuffer()
        return {"rgb": rgb, "packed": packed, "stats": stats, "work": work}

    def bind_framebuffer(self, rgb_ptr: Optional[int], packed_ptr: Optional[int]):
        self._chk(self.lib.rtx_bind_framebuffer(self.ctx, rgb_ptr, packed_ptr), "rtx_bind_framebuffer")

    def set_stream(self, stream_handle: Optional[int]):
        self._chk(self.lib.rtx_set_stream(self.ctx, stream_handle), "rtx_set_stream")
        self._stream = stream_handle

    # ---- batches of views (include/rtx.h: rtx_set_views ...) ----------------------------------------------------------------------
    def set_views(self, cameras):
        """The cameras of a batch of views of the current frame: scene_io.CAMERA (V,) or float32 (V, 12)."""
        cams = views_array(cameras)
        self._chk(self.lib.rtx_set_views(self.ctx, cams.ctypes.data, cams.shape[0]), "rtx_set_views")
        self.view_count = int(cams.shape[0])

    def _view_range(self, first_view: int, view_count: Optional[int]):
        if view_count is None:
            view_count = getattr(self, "view_count", 0) - first_view
        return int(first_view), int(view_count)

    def render_views_async(self, first_view: int = 0, view_count: Optional[int] = None, **flags):
        first_view, view_count = self._view_range(first_view, view_count)
        self._chk(self.lib.rtx_render_views(self.ctx, first_view, view_count, render_flags(**flags)), "rtx_render_views")

    def read_views(self, first_view: int = 0, view_count: Optional[int] = None):
        first_view, view_count = self._view_range(first_view, view_count)
        sc = self.scene
        rgb = np.zeros((max(view_count, 0), sc.height, sc.width, 3), np.float32)
        packed = np.zeros((max(view_count, 0), sc.height, sc.width), np.uint32)
        self._chk(self.lib.rtx_read_views(self.ctx, first_view, view_count, rgb.ctypes.data, packed.ctypes.data), "rtx_read_views")
        return rgb, packed

    def bind_view_framebuffer(self, rgb_ptr: Optional[int], packed_ptr: Optional[int], view_capacity: int = 0):
        self._chk(self.lib.rtx_bind_view_framebuffer(self.ctx, rgb_ptr, packed_ptr, view_capacity), "rtx_bind_view_framebuffer")
        self._view_fb = (rgb_ptr, packed_ptr, view_capacity) if rgb_ptr else None

    def render_views(self, first_view: int = 0, view_count: Optional[int] = None, aovs=(), **flags) -> Dict:
        """Views [first_view, first_view + view_count) of the cameras set by set_views in one rtx_render_views call (flags as render);
        rgb (V, H, W, 3) float32, packed (V, H, W) uint32, stats / work summed over the views.  Uses the context's own view framebuffer.
        aovs: AOV channel names (see bind_aovs) also returned, each (V, H, W[, k]), from the context's own AOV buffers."""
        if getattr(self, "_view_fb", None):
            self.bind_view_framebuffer(None, None)
        names = aov_names(aovs)
        if names:
            self.bind_aovs(names)
            flags = dict(flags, aov=True)
        self.render_views_async(first_view, view_count, **flags)
        stats, work = self.stats()
        rgb, packed = self.read_views(first_view, view_count)
        out = {"rgb": rgb, "packed": packed, "stats": stats, "work": work}
        if names:
            out.update(self.read_aovs(names, *self._view_range(first_view, view_count)))
        return out

    # ---- per-pixel primary-hit AOVs (include/rtx.h: rtx_bind_aovs / rtx_read_aovs) ------------------------------------------------
    def bind_aovs(self, channels, buffers: Optional[Dict] = None, pixel_capacity: int = 0):
        """Channels (RTX_AOV_* mask, a name or names: depth, position, normal, albedo, uv, material_id, object_id, triangle_id) that render
        calls with aov=True write.  buffers=None: the context's own buffers (read_aovs); else {name: device pointer} of pixel_capacity pixels
        each — a bound channel without a pointer is not written.  Empty channels unbind."""
        mask = aov_mask(channels)
        dev = None
        if buffers is not None:
            aov_names(list(buffers))
            dev = RtxAovBuffers()
            for name, ptr in buffers.items():
                setattr(dev, name, int(ptr) if ptr else None)
        self._chk(self.lib.rtx_bind_aovs(self.ctx, mask, C.byref(dev) if dev is not None else None, int(pixel_capacity)), "rtx_bind_aovs")

    def read_aovs(self, channels, first_view: int = 0, view_count: int = 1) -> Dict:
        """Pixels of views [first_view, first_view + view_count) of the context's own AOV buffers ((0, 1) = the frame of a tiles call),
        as {name: numpy array (view_count, H, W[, k])}."""
        sc = self.scene
        host = RtxAovBuffers()
        out = {}
        for name in aov_names(channels):
            a = np.zeros(aov_shape(name, view_count, sc.height, sc.width), AOV_CHANNELS[name][1])
            out[name] = a
            setattr(host, name, a.ctypes.data)
        self._chk(self.lib.rtx_read_aovs(self.ctx, first_view, view_count, C.byref(host)), "rtx_read_aovs")
        return out

    def render_aovs(self, channels=tuple(AOV_CHANNELS), **flags) -> Dict:
        """The whole frame (rtx_render_tiles with RTX_RENDER_AOV, flags as render) with the context's own AOV buffers: rgb, packed, stats,
        work and every requested channel as numpy, (H, W), (H, W, 3) or (H, W, 2)."""
        names = aov_names(channels)
        if not names:
            raise ValueError("render_aovs needs at least one AOV channel")
        self.bind_aovs(names)
        self.render_async(aov=True, **flags)
        stats, work = self.stats()
        rgb, packed = self.framebuffer()
        out = {"rgb": rgb, "packed": packed, "stats": stats, "work": work}
        out.update({name: a[0] for name, a in self.read_aovs(names, 0, 1).items()})
        return out

    def render_views_into(self, rgb, packed, first_view: int = 0, view_count: Optional[int] = None, aovs: Optional[Dict] = None, **flags):
        """Render views into caller-owned device tensors: rgb float32 (C, H, W, 3) and packed int32 (C, H, W) of C >= first_view + view_count
        views, contiguous, on this context's GPU; view v lands in rgb[v] / packed[v].  The work is queued on torch's current stream of that
        device (rtx_set_stream: the context stays on it), so torch work queued after this call sees the images.  On torch's default stream (handle 0,
        which the C ABI reads as "the context's own stream") the work goes to a side stream that waits for the current stream and that the
        current stream then waits for: the same ordering.  aovs = {channel name: tensor} also writes those per-pixel AOV channels of the
        views (see bind_aovs): float32 / int32 tensors of shape (C, H, W) or (C, H, W, k) like rgb's, checked like rgb / packed.  Returns at once."""
        first_view, view_count = self._view_range(first_view, view_count)
        self._render_into(rgb, packed, first_view, view_count, aovs, flags, lambda fl: self.render_views_async(first_view, view_count, **fl))

    def _render_into(self, rgb, packed, first_view: int, view_count: int, aovs, flags, launch, also=()):
        """render_views_into / render_rays_into: checks the output tensors, moves the context to torch's current stream, binds the tensors and
        calls launch(flags); `also` = further tensors the queued work reads."""
        import torch
        sc, dev = self.scene, self.device
        want = (("rgb", rgb, torch.float32, (sc.height, sc.width, 3)), ("packed", packed, torch.int32, (sc.height, sc.width)))
        if aovs:
            if not isinstance(aovs, dict):
                raise TypeError(f"aovs must be a dict {{channel name: tensor}}, not {type(aovs).__name__}")
            aov_names(list(aovs))
            want += tuple((name, t, torch.float32 if AOV_CHANNELS[name][1] == np.float32 else torch.int32, aov_shape(name, None, sc.height, sc.width))
                          for name, t in aovs.items())
        for name, t, dt, _ in want:
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, not {t.dtype}")
        for name, t, _, shape in want:
            if t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
                raise ValueError(f"{name} must have shape (views, {', '.join(map(str, shape))}), not {tuple(t.shape)}")
            if t.shape[0] != rgb.shape[0]:
                raise ValueError(f"rgb and {name} hold different numbers of views ({rgb.shape[0]} vs {t.shape[0]})")
        for name, t, _, _ in want:
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        for name, t, _, _ in want:
            if t.device.type != "cuda" or t.device.index != dev:
                raise ValueError(f"{name} must be on cuda:{dev} (this context's GPU), not {t.device}")
        if view_count < 1 or first_view < 0 or first_view + view_count > rgb.shape[0]:
            raise ValueError(f"views [{first_view}, {first_view + view_count}) do not fit tensors of {rgb.shape[0]} views")
        fb = (rgb.data_ptr(), packed.data_ptr(), int(rgb.shape[0]))

        def bind_and_launch():
            if getattr(self, "_view_fb", None) != fb:
                self.bind_view_framebuffer(*fb)
            fl = flags
            if aovs:
                self.bind_aovs(list(aovs), {name: t.data_ptr() for name, t in aovs.items()}, int(rgb.shape[0]) * sc.height * sc.width)
                fl = dict(flags, aov=True)
            launch(fl)
        self._on_torch_stream(bind_and_launch, tuple(w[1] for w in want) + tuple(also))

    def _on_torch_stream(self, launch, tensors):
        """Moves the context to torch's current stream of its device (rtx_set_stream: it stays there), calls launch(), and keeps `tensors`
        — everything the queued work reads or writes — from being handed out again before that work is done."""
        import torch
        dev = self.device
        cur = torch.cuda.current_stream(dev)
        # torch's default stream has the handle 0, which rtx_set_stream reads as "the context's own stream" — a non-blocking stream that does
        # not synchronise with it.  Then the work goes to a side stream of this renderer, joined to the current stream on both sides by events.
        side = None
        if cur.cuda_stream == 0:
            side = getattr(self, "_side_stream", None)
            if side is None:
                side = self._side_stream = torch.cuda.Stream(device=dev)
            side.wait_stream(cur)
        stream = (side or cur).cuda_stream
        if getattr(self, "_stream", None) != stream:
            self.set_stream(stream)
        launch()
        if side is not None:
            cur.wait_stream(side)
            for t in tensors:
                t.record_stream(side)      # the caching allocator must not hand the memory out before the work is done

    # ---- ray views: caller-supplied primary rays (include/rtx.h: rtx_set_rays / rtx_bind_rays / rtx_render_rays) -------------------
    def set_rays(self, rays):
        """The primary rays of V ray views: numpy float32 (V, H, W, 18) or (H, W, 18), row = origin, direction, dO_dx, dO_dy, dD_dx, dD_dy;
        a zero direction = no ray at that pixel.  Copied into the context's own ray buffer; a buffer bound with bind_rays is unbound."""
        r = rays_array(rays, self.scene.width, self.scene.height)
        if getattr(self, "_rays_bound", None):
            self.bind_rays(None, 0)
        self._chk(self.lib.rtx_set_rays(self.ctx, r.ctypes.data, r.shape[0]), "rtx_set_rays")
        self.ray_view_count = int(r.shape[0])

    def bind_rays(self, tensor_or_ptr, view_count: int = 0):
        """Rays in device memory: a device pointer (or an object with data_ptr(), e.g. a torch tensor) to view_count x H x W x 18 float32;
        None unbinds.  The memory stays the caller's and must outlive the work that reads it."""
        ptr = tensor_or_ptr.data_ptr() if hasattr(tensor_or_ptr, "data_ptr") else tensor_or_ptr
        self._chk(self.lib.rtx_bind_rays(self.ctx, int(ptr) if ptr else None, int(view_count)), "rtx_bind_rays")
        self._rays_bound = (int(ptr), int(view_count)) if ptr else None

    def _ray_range(self, first_view: int, view_count: Optional[int]):
        if view_count is None:
            bound = getattr(self, "_rays_bound", None)
            view_count = (bound[1] if bound else getattr(self, "ray_view_count", 0)) - first_view
        return int(first_view), int(view_count)

    def render_rays_async(self, first_view: int = 0, view_count: Optional[int] = None, **flags):
        first_view, view_count = self._ray_range(first_view, view_count)
        self._chk(self.lib.rtx_render_rays(self.ctx, first_view, view_count, render_flags(**flags)), "rtx_render_rays")

    def render_rays(self, first_view: int = 0, view_count: Optional[int] = None, aovs=(), **flags) -> Dict:
        """Ray views [first_view, first_view + view_count) of the rays set by set_rays (or bound by bind_rays) in one rtx_render_rays call
        (flags as render): rgb (V, H, W, 3) float32, packed (V, H, W) uint32, stats / work summed over the ray views, and the AOV channels
        named in aovs, each (V, H, W[, k]).  Uses the context's own view framebuffer and AOV buffers.  Pixels without a ray keep what the
        buffers held."""
        if getattr(self, "_view_fb", None):
            self.bind_view_framebuffer(None, None)
        names = aov_names(aovs)
        if names:
            self.bind_aovs(names)
            flags = dict(flags, aov=True)
        first_view, view_count = self._ray_range(first_view, view_count)
        self.render_rays_async(first_view, view_count, **flags)
        stats, work = self.stats()
        sc = self.scene
        rgb = np.zeros((max(view_count, 0), sc.height, sc.width, 3), np.float32)
        packed = np.zeros((max(view_count, 0), sc.height, sc.width), np.uint32)
        self._chk(self.lib.rtx_read_views(self.ctx, first_view, view_count, rgb.ctypes.data, packed.ctypes.data), "rtx_read_views")
        out = {"rgb": rgb, "packed": packed, "stats": stats, "work": work}
        if names:
            out.update(self.read_aovs(names, first_view, view_count))
        return out

    def render_rays_into(self, rgb, packed, rays, aovs: Optional[Dict] = None, **flags):
        """Render the ray views of `rays`, a float32 device tensor (V, H, W, 18), into caller-owned device tensors: rgb float32 (C, H, W, 3)
        and packed int32 (C, H, W) of C >= V views (ray view v lands in rgb[v] / packed[v]) and, with aovs = {channel name: tensor}, those AOV
        channels, shaped like render_views_into's.  Everything is checked (dtype, shape, contiguity, device) before the library is reached.
        Queued on torch's current stream like render_views_into; `rays` is read when the work runs and must stay alive until then.  The
        tensor is unbound again before this returns (queued work keeps the address it was launched with): a later render_rays uses the rays
        of set_rays, not memory torch may have reused.  Returns at once."""
        import torch
        sc, dev = self.scene, self.device
        if not isinstance(rays, torch.Tensor):
            raise TypeError(f"rays must be a torch.Tensor, not {type(rays).__name__}")
        if rays.dtype != torch.float32:
            raise TypeError(f"rays must be torch.float32, not {rays.dtype}")
        if rays.dim() != 4 or tuple(rays.shape[1:]) != (sc.height, sc.width, RAY_FLOATS):
            raise ValueError(f"rays must have shape (views, {sc.height}, {sc.width}, {RAY_FLOATS}), not {tuple(rays.shape)}")
        if not 1 <= rays.shape[0] <= RTX_MAX_VIEWS:
            raise ValueError(f"1 .. {RTX_MAX_VIEWS} ray views, not {rays.shape[0]}")
        if not rays.is_contiguous():
            raise ValueError("rays must be contiguous")
        if rays.device.type != "cuda" or rays.device.index != dev:
            raise ValueError(f"rays must be on cuda:{dev} (this context's GPU), not {rays.device}")
        count = int(rays.shape[0])
        self._render_into(rgb, packed, 0, count, aovs, flags, lambda fl: (self.bind_rays(rays.data_ptr(), count), self.render_rays_async(0, count, **fl), self.bind_rays(None)), (rays,))

    # ---- device-side scene update (include/rtx.h: rtx_update_instances / rtx_read_frame_state) ------------------------------------
    def update_instances(self, positions, rotations, instance_count: Optional[int] = None):
        """New poses of the frame's instances from DEVICE memory: positions (n, 3) and rotations (n, 4; quaternion x, y, z, w) as float32
        torch tensors on this context's GPU, or raw device pointers with instance_count.  The instance records and a balanced TLAS are
        rebuilt on the device, ordered on the context's stream (set_stream: torch's stream, if the tensors are written there); nothing is
        read back.  The tensors are read when the work runs and must stay alive until then.  Returns at once."""
        if hasattr(positions, "data_ptr") or hasattr(rotations, "data_ptr"):
            import torch
            for name, t, k in (("positions", positions, 3), ("rotations", rotations, 4)):
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"{name} must be a torch.Tensor (or both raw device pointers), not {type(t).__name__}")
                if t.dtype != torch.float32:
                    raise TypeError(f"{name} must be torch.float32, not {t.dtype}")
                if t.dim() != 2 or t.shape[1] != k:
                    raise ValueError(f"{name} must have shape (n, {k}), not {tuple(t.shape)}")
                if not t.is_contiguous():
                    raise ValueError(f"{name} must be contiguous")
                if t.device.type != "cuda" or t.device.index != self.device:
                    raise ValueError(f"{name} must be on cuda:{self.device} (this context's GPU), not {t.device}")
            if positions.shape[0] != rotations.shape[0]:
                raise ValueError(f"positions and rotations hold different numbers of instances ({positions.shape[0]} vs {rotations.shape[0]})")
            if instance_count is None:
                instance_count = int(positions.shape[0])
            positions, rotations = positions.data_ptr(), rotations.data_ptr()
        if instance_count is None:
            raise ValueError("instance_count is needed with raw device pointers")
        self._chk(self.lib.rtx_update_instances(self.ctx, int(positions) if positions else None, int(rotations) if rotations else None, int(instance_count)),
                  "rtx_update_instances")

    def read_frame_state(self):
        """The frame state the kernels currently read (waits for the stream): (instances scene_io.INSTANCE (n,), tlas_nodes scene_io.BVH_NODE
        in the reference layout, tlas_indices int32 (n,)) — after set_frame what was set, after update_instances what the device built."""
        nc = C.c_int32()
        self._chk(self.lib.rtx_read_frame_state(self.ctx, None, None, C.byref(nc), None), "rtx_read_frame_state")
        n = self.frame_instance_count                      # the count of the frame that was set, whichever scene object it came from
        inst = np.zeros(n, sio.INSTANCE); nodes = np.zeros(nc.value, sio.BVH_NODE); idx = np.zeros(n, np.int32)
        self._chk(self.lib.rtx_read_frame_state(self.ctx, inst.ctypes.data, nodes.ctypes.data, C.byref(nc), idx.ctypes.data), "rtx_read_frame_state")
        return inst, nodes, idx

    # ---- device-side mesh refit (include/rtx.h: rtx_bind_blas_vertices / rtx_refit_blas / rtx_read_blas) ----------------------------
    def bind_blas_vertices(self, blas_id: int, slot_vertices, vertex_count: int):
        """Once per mesh: slot_vertices (m, 3) int32 host array, the vertex indices of every flattened slot of the uploaded BLAS
        (host.slot_vertices), each in [0, vertex_count).  May allocate and wait."""
        sv = np.ascontiguousarray(slot_vertices, np.int32)
        if sv.ndim != 2 or sv.shape[1] != 3:
            raise ValueError(f"slot_vertices must have shape (slots, 3), not {tuple(sv.shape)}")
        if 0 <= blas_id < len(self._blas_shapes) and self._blas_shapes[blas_id] and sv.shape[0] != self._blas_shapes[blas_id][1]:
            raise ValueError(f"slot_vertices holds {sv.shape[0]} slots, BLAS {blas_id} {self._blas_shapes[blas_id][1]}")
        self._chk(self.lib.rtx_bind_blas_vertices(self.ctx, int(blas_id), sv.ctypes.data, int(vertex_count)), "rtx_bind_blas_vertices")

    def refit_blas(self, blas_id: int, positions, normals=None, vertex_count: Optional[int] = None):
        """New vertex positions (V, 3) — and normals (V, 3), or None: the normals stay — of a bound mesh from DEVICE memory: float32 torch
        tensors on this context's GPU, or raw device pointers with vertex_count.  Triangles, boxes and plane lists of the BLAS are rewritten in
        place, ordered on the context's stream; nothing is read back.  The tensors are read when the work runs and must stay alive until
        then.  Returns at once.  The TLAS is not touched: follow with update_instances when the mesh's root box moves."""
        if hasattr(positions, "data_ptr") or hasattr(normals, "data_ptr"):
            import torch
            for name, t in (("positions", positions), ("normals", normals)):
                if t is None and name == "normals":
                    continue
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"{name} must be a torch.Tensor (or raw device pointers), not {type(t).__name__}")
                if t.dtype != torch.float32:
                    raise TypeError(f"{name} must be torch.float32, not {t.dtype}")
                if t.dim() != 2 or t.shape[1] != 3:
                    raise ValueError(f"{name} must have shape (V, 3), not {tuple(t.shape)}")
                if not t.is_contiguous():
                    raise ValueError(f"{name} must be contiguous")
                if t.device.type != "cuda" or t.device.index != self.device:
                    raise ValueError(f"{name} must be on cuda:{self.device} (this context's GPU), not {t.device}")
            if normals is not None and normals.shape[0] != positions.shape[0]:
                raise ValueError(f"positions and normals hold different numbers of vertices ({positions.shape[0]} vs {normals.shape[0]})")
            if vertex_count is None:
                vertex_count = int(positions.shape[0])
            positions, normals = positions.data_ptr(), (None if normals is None else normals.data_ptr())
        if vertex_count is None:
            raise ValueError("vertex_count is needed with raw device pointers")
        self._chk(self.lib.rtx_refit_blas(self.ctx, int(blas_id), int(positions) if positions else None, int(normals) if normals else None, int(vertex_count)),
                  "rtx_refit_blas")

    # ---- device-side mesh build (include/rtx.h: rtx_alloc_blas / rtx_build_blas) -----------------------------------------------------
    def alloc_blas(self, blas_id: int, triangle_count: int, vertex_count: int, material_ids=None, material_offset: int = 0):
        """Once per mesh: a BLAS of up to triangle_count triangles over vertex_count vertices under blas_id, with the balanced tree's topology
        (host.blas_build_balanced documents it) and every buffer a build needs.  material_ids: one local id per source triangle (host array,
        each >= 0), None = all 0.  Until the first build_blas the mesh is empty and legal to render.  May allocate and wait."""
        from . import host
        mids = None
        if material_ids is not None:
            mids = np.ascontiguousarray(material_ids, np.int32)
            if mids.shape != (int(triangle_count),):
                raise ValueError(f"material_ids must have shape ({int(triangle_count)},), not {tuple(mids.shape)}")
        self._chk(self.lib.rtx_alloc_blas(self.ctx, int(blas_id), int(triangle_count), int(vertex_count), None if mids is None else mids.ctypes.data,
                                          int(material_offset)), "rtx_alloc_blas")
        self._blas_shapes += [None] * (blas_id + 1 - len(self._blas_shapes))
        self._blas_shapes[blas_id] = (host.blas_balanced_node_count(int(triangle_count)), int(triangle_count), int(material_offset), int(triangle_count))
        self._built_shapes = getattr(self, "_built_shapes", {})
        self._built_shapes[int(blas_id)] = (int(triangle_count), int(vertex_count))

    def build_blas(self, blas_id: int, positions, indices, normals, texcoords=None, order_out=None):
        """The mesh of an alloc_blas id rebuilt from DEVICE memory: positions (V, 3) f32, indices (T, 3) i32, normals (V, 3) f32, texcoords
        (V, 2) f32 or None (zeros), order_out (T,) i32 or None (receives the source triangle of every flattened slot: what the triangle_id AOV
        reports) — torch tensors on this context's GPU with the T and V of alloc_blas, or raw device pointers.  A triangle with an index
        outside [0, V) is invalid (-1 pads a mesh with fewer triangles).  Ordered on the context's stream; nothing is read back.  The tensors are
        read when the work runs and must stay alive until then.  Returns at once.  The TLAS is not touched: follow with update_instances.
        Afterwards refit_blas(blas_id, positions, normals) moves the vertices in the tree of the last build."""
        args = (("positions", positions, 3, "float32"), ("indices", indices, 3, "int32"), ("normals", normals, 3, "float32"),
                ("texcoords", texcoords, 2, "float32"), ("order_out", order_out, 0, "int32"))
        ptrs = []
        if any(hasattr(t, "data_ptr") for _, t, _, _ in args):
            import torch
            T, V = getattr(self, "_built_shapes", {}).get(int(blas_id), (None, None))
            for name, t, k, dt in args:
                if t is None and name in ("texcoords", "order_out"):
                    ptrs.append(None); continue
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"{name} must be a torch.Tensor (or all raw device pointers), not {type(t).__name__}")
                if t.dtype != getattr(torch, dt):
                    raise TypeError(f"{name} must be torch.{dt}, not {t.dtype}")
                rows = T if name in ("indices", "order_out") else V
                if (t.dim() != 2 or t.shape[1] != k) if k else t.dim() != 1:
                    raise ValueError(f"{name} must have shape ({'T' if name in ('indices', 'order_out') else 'V'}{', %d' % k if k else ''}), not {tuple(t.shape)}")
                if rows is not None and t.shape[0] != rows:
                    raise ValueError(f"{name} holds {t.shape[0]} rows, alloc_blas was given {rows}")
                if not t.is_contiguous():
                    raise ValueError(f"{name} must be contiguous")
                if t.device.type != "cuda" or t.device.index != self.device:
                    raise ValueError(f"{name} must be on cuda:{self.device} (this context's GPU), not {t.device}")
                ptrs.append(t.data_ptr())
        else:
            ptrs = [int(t) if t else None for _, t, _, _ in args]
        self._chk(self.lib.rtx_build_blas(self.ctx, int(blas_id), *ptrs), "rtx_build_blas")

    # ---- device-side vertex normals (include/rtx.h: rtx_alloc_blas_topology / rtx_set_blas_topology / rtx_blas_vertex_normals) ----------
    def _normals_tensor(self, name: str, t, dtype: str, rows: Optional[int] = None, letter: str = "V"):
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype != getattr(torch, dtype):
            raise TypeError(f"{name} must be torch.{dtype}, not {t.dtype}")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} must have shape ({letter}, 3), not {tuple(t.shape)}")
        if rows is not None and t.shape[0] != rows:
            raise ValueError(f"{name} holds {t.shape[0]} rows, set_blas_topology was given {rows}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError(f"{name} must be on cuda:{self.device} (this context's GPU), not {t.device}")

    def set_blas_topology(self, blas_id: int, indices, vertex_count: int):
        """The SOURCE index buffer of the mesh under blas_id, for vertex_normals: indices (T, 3) int32 torch tensor on this context's GPU
        over vertex_count vertices; a triangle with an index outside [0, vertex_count) is invalid and contributes to no vertex (-1 pads).
        Once for a refitted mesh, every step for a rebuilt one.  The first call for an id, or one with other counts, allocates (and may
        wait); otherwise the inverted index is rebuilt on the context's stream and nothing is read back.  The tensor is read when the
        work runs and must stay alive until then."""
        self._normals_tensor("indices", indices, "int32", letter="T")
        T, V = int(indices.shape[0]), int(vertex_count)
        if T < 1 or V < 1:
            raise ValueError(f"indices must hold at least one triangle and vertex_count must be at least 1, not {T} and {V}")
        shapes = self.__dict__.setdefault("_topology_shapes", {})
        rc = RTX_ERR_STATE
        if shapes.get(int(blas_id)) == (T, V):       # an upload or alloc_blas over the id has dropped the topology: RTX_ERR_STATE, allocate again
            rc = self.lib.rtx_set_blas_topology(self.ctx, int(blas_id), indices.data_ptr())
        if rc == RTX_ERR_STATE:
            shapes.pop(int(blas_id), None)
            self.__dict__.setdefault("_normals_out", {}).pop(int(blas_id), None)
            self._chk(self.lib.rtx_alloc_blas_topology(self.ctx, int(blas_id), T, V), "rtx_alloc_blas_topology")
            shapes[int(blas_id)] = (T, V)
            rc = self.lib.rtx_set_blas_topology(self.ctx, int(blas_id), indices.data_ptr())
        self._chk(rc, "rtx_set_blas_topology")

    def vertex_normals(self, blas_id: int, positions, out=None):
        """Smooth, area-weighted vertex normals of the topology set under blas_id at the positions (V, 3) float32 torch tensor on this
        context's GPU, written to out (V, 3) float32 — None: a tensor this Renderer owns per id, made once and reused — and returned, so
        that r.refit_blas(i, pos, r.vertex_normals(i, pos)) is the whole step.  Bit-reproducible and bit-identical to host.vertex_normals;
        a vertex no valid triangle uses, or whose face vectors cancel, gets (0, 0, 0).  Ordered on the context's stream; nothing is read
        back.  The tensors are read and written when the work runs and must stay alive until then.  Returns at once."""
        T, V = getattr(self, "_topology_shapes", {}).get(int(blas_id), (None, None))
        self._normals_tensor("positions", positions, "float32", V)
        if out is None:
            import torch
            owned = self.__dict__.setdefault("_normals_out", {})
            out = owned.get(int(blas_id))
            if out is None or out.shape != positions.shape:
                out = owned[int(blas_id)] = torch.empty_like(positions)
        else:
            self._normals_tensor("out", out, "float32", int(positions.shape[0]))
        self._chk(self.lib.rtx_blas_vertex_normals(self.ctx, int(blas_id), positions.data_ptr(), out.data_ptr()), "rtx_blas_vertex_normals")
        return out

    # ---- pseudonormal tables (include/rtx.h: rtx_blas_pseudonormals / rtx_read_blas_pseudonormals) --------------------------------------
    def blas_pseudonormals(self, blas_id: int, positions):
        """The angle-weighted pseudonormal tables of the mesh under blas_id at the positions (V, 3) float32 torch tensor on this context's
        GPU (or a raw device pointer), which query_signed_distance reads near edges and vertices.  Needs set_blas_topology (the SOURCE
        indices) and bound slot vertices (bind_blas_vertices, or alloc_blas + build_blas), over the same V.  The first call for an id
        allocates and may wait; later calls are queued on the context's stream and read nothing back.  The per-step idiom:
        r.refit_blas(i, pos, r.vertex_normals(i, pos)); r.blas_pseudonormals(i, pos).  The tables are as current as the last call."""
        if hasattr(positions, "data_ptr"):
            T, V = getattr(self, "_topology_shapes", {}).get(int(blas_id), (None, None))
            self._normals_tensor("positions", positions, "float32", V)
            positions = positions.data_ptr()
        self._chk(self.lib.rtx_blas_pseudonormals(self.ctx, int(blas_id), int(positions) if positions else None), "rtx_blas_pseudonormals")

    def read_blas_pseudonormals(self, blas_id: int):
        """The tables the kernels currently read (waits for the stream) -> (vert (V, 4), edge (slots, 3, 4)) float32: what
        host.blas_pseudonormals computes from the same positions, indices and slot vertices, bit for bit."""
        T, V = getattr(self, "_topology_shapes", {}).get(int(blas_id), (None, None))
        if V is None or not (0 <= blas_id < len(self._blas_shapes)) or not self._blas_shapes[blas_id]:
            self._chk(self.lib.rtx_read_blas_pseudonormals(self.ctx, int(blas_id), None, None), "rtx_read_blas_pseudonormals")
            raise ValueError(f"BLAS {blas_id} has no topology set through this Renderer")
        slots = self._blas_shapes[blas_id][1]
        vert = np.zeros((V, 4), np.float32); edge = np.zeros((slots, 3, 4), np.float32)
        self._chk(self.lib.rtx_read_blas_pseudonormals(self.ctx, int(blas_id), vert.ctypes.data, edge.ctypes.data), "rtx_read_blas_pseudonormals")
        return vert, edge

    def read_blas(self, blas_id: int) -> sio.Blas:
        """The BLAS arrays the kernels currently read (waits for the stream): after upload what was uploaded, after refit_blas what the device
        wrote."""
        if not (0 <= blas_id < len(self._blas_shapes)) or not self._blas_shapes[blas_id]:
            self._chk(self.lib.rtx_read_blas(self.ctx, int(blas_id), None, None, None), "rtx_read_blas")
            raise ValueError(f"BLAS {blas_id} was not uploaded through this Renderer")
        n, m, off, src = self._blas_shapes[blas_id]
        nodes = np.zeros(n, sio.BVH_NODE); hot = np.zeros(m, sio.TRI_HOT); cold = np.zeros(m, sio.TRI_COLD)
        self._chk(self.lib.rtx_read_blas(self.ctx, int(blas_id), nodes.ctypes.data, hot.ctypes.data, cold.ctypes.data), "rtx_read_blas")
        return sio.Blas(nodes, hot, cold, off, src)

    # ---- device-side texture and sky update (include/rtx.h: rtx_alloc_texture / rtx_update_texture / rtx_read_texture / rtx_update_sky) ----
    def alloc_texture(self, texture_id: int, width: int, height: int, mipmapped: Optional[bool] = None):
        """Once per texture: a zeroed width x height texture under texture_id whose texels update_texture rewrites from device memory, with
        the mip chain Texture::load would give it when mipmapped (None: the scene's texture_mode is the mipmap mode) and both sides are powers
        of two.  May allocate and wait."""
        if mipmapped is None:
            mipmapped = int(self.scene.config["texture_mode"][0]) == 2
        self._chk(self.lib.rtx_alloc_texture(self.ctx, int(texture_id), int(width), int(height), 1 if mipmapped else 0), "rtx_alloc_texture")

    def _texture_shape(self, texture_id: int):
        """(H, W) of the texture the context holds under texture_id, however it got there (the library's own descriptor: nothing waits), or
        None when the id holds nothing."""
        desc = RtxTextureDesc()
        if self.lib.rtx_read_texture(self.ctx, int(texture_id), C.byref(desc), None, 0):
            return None
        return (int(desc.height), int(desc.width))

    @staticmethod
    def _texel_tensor(name: str, t, device: int, shape=None) -> int:
        """The RTX_TEXELS_* format of a texel tensor ((H, W, 3) float32 or (H, W, 4) uint8, contiguous, on cuda:device, of `shape` = (H, W) when
        given); ValueError before anything reaches the library."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{name} must be torch.float32 (H, W, 3) or torch.uint8 (H, W, 4), not {t.dtype}")
        channels = 3 if t.dtype == torch.float32 else 4
        if t.dim() != 3 or t.shape[2] != channels or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{name} of {t.dtype} must have shape (H, W, {channels}), not {tuple(t.shape)}")
        if shape is not None and tuple(t.shape[:2]) != tuple(shape):
            raise ValueError(f"{name} must be ({shape[0]}, {shape[1]}, {channels}), the size of the texture, not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError(f"{name} must be on cuda:{device} (this context's GPU), not {t.device}")
        return RTX_TEXELS_RGB_F32 if t.dtype == torch.float32 else RTX_TEXELS_RGBA8_SRGB

    def update_texture(self, texture_id: int, tensor):
        """New texels of an alloc_texture id from DEVICE memory: a contiguous torch tensor on this context's GPU of the allocated size, (H, W, 3)
        float32 in linear light (what render_views_into leaves in rgb[v]) or (H, W, 4) uint8 sRGB r, g, b, a (alpha dropped).  Level 0 and the
        whole mip chain are rewritten in place, queued on torch's current stream like render_views_into; nothing is read back and no graph is
        invalidated.  The tensor is read when the work runs.  Returns at once."""
        fmt = self._texel_tensor("tensor", tensor, self.device, self._texture_shape(texture_id))      # no texture under the id: the library says so
        self._on_torch_stream(lambda: self._chk(self.lib.rtx_update_texture(self.ctx, int(texture_id), tensor.data_ptr(), fmt), "rtx_update_texture"), (tensor,))

    def read_texture(self, texture_id: int) -> sio.Texture:
        """The descriptor and the texels (chain included, (n, 3) float32) the samplers currently read under an uploaded or allocated id
        (waits for the stream)."""
        desc = RtxTextureDesc()
        self._chk(self.lib.rtx_read_texture(self.ctx, int(texture_id), C.byref(desc), None, 0), "rtx_read_texture")
        count = max(desc.mip_offsets[l] + (desc.width >> l) * (desc.height >> l) for l in range(desc.mip_levels))
        texels = np.zeros((count, 3), np.float32)
        self._chk(self.lib.rtx_read_texture(self.ctx, int(texture_id), C.byref(desc), texels.ctypes.data, count), "rtx_read_texture")
        d = np.zeros(1, sio.TEXTURE_DESC)
        C.memmove(d.ctypes.data, C.byref(desc), C.sizeof(desc))
        return sio.Texture(d, texels)

    def update_sky(self, tensor):
        """New texels of the uploaded sky probe from DEVICE memory: a contiguous (S, S, 3) float32 torch tensor on this context's GPU, S the
        uploaded size.  One device-to-device copy queued on torch's current stream.  Returns at once."""
        import torch
        if isinstance(tensor, torch.Tensor) and (tensor.dtype != torch.float32 or tensor.dim() != 3 or tensor.shape[0] != tensor.shape[1] or tensor.shape[2] != 3):
            raise ValueError(f"the sky must be (S, S, 3) torch.float32, not {tuple(tensor.shape)} {tensor.dtype}")
        self._texel_tensor("tensor", tensor, self.device)
        self._on_torch_stream(lambda: self._chk(self.lib.rtx_update_sky(self.ctx, tensor.data_ptr(), int(tensor.shape[0])), "rtx_update_sky"), (tensor,))

    def debug_read_layouts(self, blas_id: int = -1) -> Dict:
        """The node layouts derived from the lane layout, as the kernels read them now (rtx_debug_read_layouts; waits for the stream), as
        uint32 bit patterns.  A BLAS id: {"pk": (n, 8), "pk4": (2n + 4, 8) or None, "pk4c": (2n + 4, 8) or None, "planes": [x, y, z]} — a
        row is (min.x, min.y, max.x, max.y, min.z, max.z, first, count / meta), None = the mesh keeps that binary walk.  -1: {"pk": (n, 8)}
        of the current frame's TLAS."""
        info = np.zeros(8, np.int32)
        self._chk(self.lib.rtx_debug_read_layouts(self.ctx, int(blas_id), info.ctypes.data, None, None, None, None, None, None), "rtx_debug_read_layouts")
        n = int(info[0])
        pk = np.zeros((n, 8), np.uint32)
        if blas_id < 0:
            self._chk(self.lib.rtx_debug_read_layouts(self.ctx, int(blas_id), None, pk.ctypes.data, None, None, None, None, None), "rtx_debug_read_layouts")
            return {"pk": pk}
        pk4 = np.zeros((2 * n + 4, 8), np.uint32) if info[1] else None
        pk4c = np.zeros((2 * n + 4, 8), np.uint32) if info[2] else None
        planes = [np.zeros(int(info[3 + a]), np.uint32) for a in range(3)]
        self._chk(self.lib.rtx_debug_read_layouts(self.ctx, int(blas_id), None, pk.ctypes.data, None if pk4 is None else pk4.ctypes.data,
                                                  None if pk4c is None else pk4c.ctypes.data, *(p.ctypes.data if p.size else None for p in planes)),
                  "rtx_debug_read_layouts")
        return {"pk": pk, "pk4": pk4, "pk4c": pk4c, "planes": planes}

    # ---- ray queries (include/rtx.h: rtx_query_closest / rtx_query_occluded) ---------------------------------------------------------
    GRID_NAMES = ("cus", "trace_blocks_closest", "trace_blocks_any", "trace_blocks_count", "pk_blocks_closest", "pk_blocks_any", "item_blocks",
                  "spill_threads")

    def debug_grids(self) -> np.ndarray:
        """The grids this context launches (rtx_debug_grids), in GRID_NAMES order: the compute units they are sized for (RTX_GRID_CUS, else the
        device's), the workgroups of the per-lane closest-hit, per-lane shadow-ray and plain traversal launches (256 threads each), of the
        closest-hit and shadow-ray packet launches and of the item launch (one wave each), and the threads the spill regions hold."""
        out = np.zeros(8, np.int32)
        self._chk(self.lib.rtx_debug_grids(self.ctx, out.ctypes.data), "rtx_debug_grids")
        return out

    def _query_rows(self, name: str, rows, width: int, n: Optional[int]):
        """(device pointer, n, tensor or None) of a query's input: a float32 torch tensor (n, width), or a raw device pointer with n.
        Raises before anything reaches the library; _query_on_device checks where the tensor lives."""
        if isinstance(rows, (int, np.integer)) and not isinstance(rows, bool):
            if n is None:
                raise ValueError(f"n is needed when {name} is a raw device pointer")
            if int(n) < 1 or not rows:
                raise ValueError(f"{name}: a non-null device pointer and n >= 1 are needed, not {rows} and {n}")
            return int(rows), int(n), None
        import torch
        if not isinstance(rows, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor (or a raw device pointer with n), not {type(rows).__name__}")
        if rows.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, not {rows.dtype}")
        if rows.dim() != 2 or rows.shape[1] != width:
            raise ValueError(f"{name} must have shape (n, {width}), not {tuple(rows.shape)}")
        if not rows.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if n is None:
            n = int(rows.shape[0])
        if not 1 <= int(n) <= rows.shape[0]:
            raise ValueError(f"n must be in [1, {rows.shape[0]}] for {name} of shape {tuple(rows.shape)}, not {n}")
        return rows.data_ptr(), int(n), rows

    @staticmethod
    def _query_shape(n: int, k: int, hits: int = 0) -> tuple:
        """Shape of a query channel of width k: (n,) or (n, k); with `hits` entries per row (query_hits) (n, hits) or (n, hits, k)."""
        return (n,) + ((hits,) if hits else ()) + ((k,) if k > 1 else ())

    def _query_out(self, name: str, t, dtype, n: int, k: int, raw: bool, hits: int = 0):
        """Device pointer of an output: a caller tensor of n rows (checked; `hits` entries per row for query_hits), or with raw inputs a
        raw device pointer."""
        if raw and isinstance(t, (int, np.integer)) and not isinstance(t, bool):
            if not t:
                raise ValueError(f"out[{name!r}] is a null device pointer")
            return int(t)
        import torch
        want_dt = torch.float32 if dtype == np.float32 else torch.int32
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"out[{name!r}] must be a torch.Tensor, not {type(t).__name__}")
        if t.dtype != want_dt:
            raise TypeError(f"out[{name!r}] must be {want_dt}, not {t.dtype}")
        shape = self._query_shape(n, k, hits)
        if tuple(t.shape) != shape:
            raise ValueError(f"out[{name!r}] must have shape {shape}, not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be contiguous")
        return t.data_ptr()

    def _query_on_device(self, tensors: Dict):
        """The last check of a query, after every type, dtype and shape: each tensor lives on this context's GPU."""
        for name, t in tensors.items():
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError(f"{name} must be on cuda:{self.device} (this context's GPU), not {t.device}")

    def query_closest(self, rays, channels=("distance",), out: Optional[Dict] = None, n: Optional[int] = None, sort: bool = False, **flags) -> Dict:
        """The closest hit of n arbitrary rays against the frame the context holds (rtx_query_closest): rays = float32 torch tensor (n, 6)
        of (origin, direction) on this context's GPU; channels = names out of distance, position, normal, uv, material_id, object_id,
        triangle_id (or a RTX_QUERY_* mask).  Returns {name: tensor}: float32 / int32, (n,), (n, 3) or (n, 2), allocated on the device unless
        out = {name: tensor} supplies them.  A miss: distance inf, ids -1, the rest 0; a zero direction is no ray and a miss.  Queued on
        torch's current stream like render_views_into: torch work queued after the call sees the answers, nothing is read back.  flags:
        lane_trace / packet_closest.  sort=True (RTX_QUERY_SORT): the library sorts the rays of every round into coherent packets on the
        device and scatters the answers back; the same answers, row for row.  Raw device pointers: rays = address, n = rays, out = {name: address} for every channel wanted (then the
        work goes to the stream set with set_stream).  Everything is checked before the library is reached.  Returns at once."""
        names = query_names(channels)
        ptr, n, rays_t = self._query_rows("rays", rays, 6, n)
        if out is not None and not isinstance(out, dict):
            raise TypeError(f"out must be a dict {{channel name: tensor}}, not {type(out).__name__}")
        out = dict(out or {})
        query_names(list(out) or names)
        extra = [k for k in out if k not in names]
        if extra:
            raise ValueError(f"out holds channels that were not requested: {', '.join(extra)}")
        raw = rays_t is None
        if raw and len(out) != len(names):
            raise ValueError("with raw device pointers out must hold an address for every requested channel")
        fl = render_flags(**flags)
        if fl & ~(RTX_RENDER_LANE_TRACE | RTX_RENDER_PACKET_CLOSEST):
            raise ValueError("a query takes the flags lane_trace and packet_closest only")
        if sort:
            fl |= RTX_QUERY_SORT
        buf = RtxQueryBuffers()
        for name in out:
            _, dt, k = QUERY_CHANNELS[name]
            setattr(buf, name, self._query_out(name, out[name], dt, n, k, raw))
        self._query_on_device({k: t for k, t in [("rays", rays_t)] + [(f"out[{k!r}]", t) for k, t in out.items()] if hasattr(t, "device")})
        for name in names:
            if name not in out:
                import torch
                _, dt, k = QUERY_CHANNELS[name]
                out[name] = torch.empty((n, k) if k > 1 else (n,), dtype=torch.float32 if dt == np.float32 else torch.int32, device=rays_t.device)
                setattr(buf, name, out[name].data_ptr())
        mask = sum(QUERY_CHANNELS[name][0] for name in names)

        def launch():
            self._chk(self.lib.rtx_query_closest(self.ctx, ptr, n, mask, C.byref(buf), fl), "rtx_query_closest")
        tensors = [t for t in [rays_t] + list(out.values()) if hasattr(t, "record_stream")]
        if tensors:
            self._on_torch_stream(launch, tensors)
        else:
            launch()
        return {name: out[name] for name in names}

    def query_occluded(self, segments, out=None, n: Optional[int] = None, sort: bool = False, **flags):
        """Whether each of n segments is blocked (rtx_query_occluded): segments = float32 torch tensor (n, 7) of (origin, direction, max
        distance) on this context's GPU; returns the int32 tensor (n,) of 1 / 0 (out, or a new one): 1 = something is hit at a distance
        strictly below the maximum.  Queued, checked and flagged like query_closest; raw device pointers: segments = address, n, out = address."""
        ptr, n, seg_t = self._query_rows("segments", segments, 7, n)
        raw = seg_t is None
        fl = render_flags(**flags)
        if fl & ~(RTX_RENDER_LANE_TRACE | RTX_RENDER_PACKET_CLOSEST):
            raise ValueError("a query takes the flags lane_trace and packet_closest only")
        if sort:
            fl |= RTX_QUERY_SORT
        if out is None and raw:
            raise ValueError("with raw device pointers out must be the address of the result")
        optr = None if out is None else self._query_out("occluded", out, np.int32, n, 1, raw)
        self._query_on_device({k: t for k, t in (("segments", seg_t), ("out", out)) if hasattr(t, "device")})
        if out is None:
            import torch
            out = torch.empty((n,), dtype=torch.int32, device=seg_t.device)
            optr = out.data_ptr()

        def launch():
            self._chk(self.lib.rtx_query_occluded(self.ctx, ptr, n, optr, fl), "rtx_query_occluded")
        tensors = [t for t in (seg_t, out) if hasattr(t, "record_stream")]
        if tensors:
            self._on_torch_stream(launch, tensors)
        else:
            launch()
        return out

    # ---- object masks: the filtered walk queries (include/rtx.h: rtx_set_object_masks ... rtx_query_*_filtered) ---------------------
    def set_object_masks(self, masks):
        """The object masks the filtered queries (mask=...) test: one 32-bit mask per object of the current frame, instances first, then
        spheres, then planes (the numbering of the object_id channel).  A numpy array goes through rtx_set_object_masks (a staged copy on
        the context's stream); a torch tensor on this context's GPU through rtx_update_object_masks (device to device, queued on torch's
        current stream, nothing read back).  int32 and uint32 are both accepted and the bits taken as they are (torch has no general
        uint32).  None drops the table: every object's mask is all ones again.  An object exists for a row iff object mask & row mask != 0."""
        if masks is None:
            self._chk(self.lib.rtx_set_object_masks(self.ctx, None, 0), "rtx_set_object_masks")
            return
        if hasattr(masks, "data_ptr"):
            import torch
            if not isinstance(masks, torch.Tensor):
                raise TypeError(f"masks must be a numpy array, a torch.Tensor or None, not {type(masks).__name__}")
            if masks.dtype not in (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()):
                raise TypeError(f"masks must be torch.int32 (or uint32), not {masks.dtype}")
            if masks.dim() != 1:
                raise ValueError(f"masks must have shape (M,), not {tuple(masks.shape)}")
            if not masks.is_contiguous():
                raise ValueError("masks must be contiguous")
            self._query_on_device({"masks": masks})
            count = int(masks.shape[0])
            self._on_torch_stream(lambda: self._chk(self.lib.rtx_update_object_masks(self.ctx, masks.data_ptr() if count else None, count), "rtx_update_object_masks"), [masks])
            return
        a = np.asarray(masks)
        if a.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
            raise TypeError(f"masks must be int32 or uint32, not {a.dtype}")
        if a.ndim != 1:
            raise ValueError(f"masks must have shape (M,), not {a.shape}")
        a = np.ascontiguousarray(a)
        keep = a if len(a) else np.zeros(1, np.uint32)      # M = 0 with an array: an empty table, not a dropped one
        self._chk(self.lib.rtx_set_object_masks(self.ctx, keep.ctypes.data, len(a)), "rtx_set_object_masks")

    def read_object_masks(self) -> Optional[np.ndarray]:
        """The object masks the kernels see (rtx_read_object_masks; waits for the stream): uint32 (M,), or None when there is no table."""
        cnt = C.c_int32()
        self._chk(self.lib.rtx_read_object_masks(self.ctx, None, 0, C.byref(cnt)), "rtx_read_object_masks")
        if cnt.value == 0:
            return None
        out = np.zeros(cnt.value, np.uint32)
        self._chk(self.lib.rtx_read_object_masks(self.ctx, out.ctypes.data, cnt.value, C.byref(cnt)), "rtx_read_object_masks")
        return out[:cnt.value]

    def _query_filter(self, mask, n: int):
        """(RtxQueryFilter or None, the row-mask tensor or None) of a query's mask keyword: None = the unfiltered call; an int = that mask for
        every row; an int32 torch tensor (n,) on this context's GPU = the row masks; with raw device pointers an ("address", ptr) is not
        offered: pass a tensor."""
        if mask is None:
            return None, None
        if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool):
            if not -(1 << 31) <= int(mask) <= 0xFFFFFFFF:
                raise ValueError(f"mask {mask} does not fit 32 bits")
            return RtxQueryFilter(None, int(mask) & 0xFFFFFFFF), None
        import torch
        if not isinstance(mask, torch.Tensor):
            raise TypeError(f"mask must be None, an int or a torch.Tensor of row masks, not {type(mask).__name__}")
        if mask.dtype not in (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()):
            raise TypeError(f"mask must be torch.int32 (or uint32), not {mask.dtype}")
        if tuple(mask.shape) != (n,):
            raise ValueError(f"mask must have shape ({n},), not {tuple(mask.shape)}")
        if not mask.is_contiguous():
            raise ValueError("mask must be contiguous")
        self._query_on_device({"mask": mask})
        return RtxQueryFilter(mask.data_ptr(), 0), mask

    def query_nearest(self, points, channels=("distance",), out: Optional[Dict] = None, n: Optional[int] = None, sort: bool = False, mask=None) -> Dict:
        """The nearest surface point of n points against the frame the context holds (rtx_query_nearest): points = float32 torch tensor
        (n, 4) of (x, y, z, maximum distance) on this context's GPU; channels as for query_closest.  Returns {name: tensor}: distance to the
        nearest surface point, that point, and what a hit there would report as normal, uv and ids.  No answer (nothing strictly nearer
        than the maximum distance, a non-finite coordinate, a maximum distance that is NaN or not above 0): distance inf, ids -1, the rest 0;
        +inf is a legal maximum distance.  Distances are measured in each instance's local space, so the frame's instances must be rigid poses
        (a scaled, sheared or flattened matrix: RtxError, RTX_ERR_STATE — on every length query: this one, query_signed_distance, query_sweep,
        query_overlap, query_overlapped, query_overlap_capsule, query_overlapped_capsule, query_sweep_box; query_hits, query_closest and query_occluded take any finite matrix).  Queued on torch's current stream, checked
        and shaped like query_closest; sort=True (RTX_QUERY_SORT) walks the points of every round in Morton order, same answers row for row.
        Raw device pointers: points = address, n, out = {name: address} for every channel wanted.
        mask (here, on query_hits and on query_sweep): None = this call; an int = the row mask of every row; an int32 tensor (n,) on this
        context's GPU = one mask per row.  A row sees the objects whose mask (set_object_masks; all ones without a table) shares a bit with
        its own; a row whose mask is 0 gets the no-answer values (rtx_query_*_filtered)."""
        return self._query_rows_to_channels("rtx_query_nearest", "points", points, 4, channels, out, n, sort, mask)

    def query_signed_distance(self, points, channels=(), out: Optional[Dict] = None, n: Optional[int] = None, sort: bool = False, mask=None,
                              feature: bool = False) -> Dict:
        """query_nearest with a sign (rtx_query_signed_distance): returns {"signed_distance": (n,) float32[, "feature": (n,) int32], and
        the requested channels of query_nearest, bit for bit}.  The distance is negative where the point lies behind the surface: for a
        closed, outward-oriented mesh inside it; for an open one (a cloth) below it.  The side is decided by the angle-weighted pseudonormal
        of the face, edge or vertex that holds the nearest point (blas_pseudonormals makes the tables), so it is right near convex and
        concave edges and vertices, where the nearest triangle's face normal is not.  Spheres are negative inside, planes on the side
        their normal points away from; a row without an answer gets +inf; a point on the surface +0.  feature: 0 none, 1 face, 2 edge,
        3 vertex, 4 sphere, 5 plane, + 8 when the winning mesh has no tables (the face rule everywhere).  The sign is relative to the object
        that owns the nearest point, not to a union of overlapping solids.  Checked, shaped and queued like query_nearest; channels may be
        empty.  out may hold "signed_distance" and "feature" tensors too.  Raw device pointers: points = address, n, out = {name: address}
        for "signed_distance", for "feature" when wanted, and for every channel."""
        return self._query_rows_to_channels("rtx_query_nearest", "points", points, 4, channels, out, n, sort, mask, signed={"feature": bool(feature)})

    def _query_rows_to_channels(self, fn, label, rows, width, channels, out, n, sort, mask=None, signed=None) -> Dict:
        """query_nearest and query_sweep: rows of `width` floats in, one element of every requested channel per row out.  signed (a dict):
        query_signed_distance — the channels may be empty, and "signed_distance" (and "feature") come first in the result."""
        if signed is not None and not isinstance(channels, (str, int, np.integer)) and len(tuple(channels)) == 0:
            names = ()
        else:
            names = query_names(channels)
        side = {} if signed is None else {"signed_distance": np.float32, **({"feature": np.int32} if signed["feature"] else {})}
        if out is not None and isinstance(out, dict):
            side_out = {k: out[k] for k in side if k in out}
            out = {k: v for k, v in out.items() if k not in side}
        else:
            side_out = {}
        ptr, n, pts_t = self._query_rows(label, rows, width, n)
        if out is not None and not isinstance(out, dict):
            raise TypeError(f"out must be a dict {{channel name: tensor}}, not {type(out).__name__}")
        out = dict(out or {})
        if out or names:
            query_names(list(out) or names)
        extra = [k for k in out if k not in names]
        if extra:
            raise ValueError(f"out holds channels that were not requested: {', '.join(extra)}")
        raw = pts_t is None
        if raw and (len(out) != len(names) or len(side_out) != len(side)):
            raise ValueError("with raw device pointers out must hold an address for every requested channel")
        fl = RTX_QUERY_SORT if sort else 0
        filt, mask_t = self._query_filter(mask, n)
        side_ptr = {k: self._query_out(k, t, side[k], n, 1, raw) for k, t in side_out.items()}
        buf = RtxQueryBuffers()
        for name in out:
            _, dt, k = QUERY_CHANNELS[name]
            setattr(buf, name, self._query_out(name, out[name], dt, n, k, raw))
        self._query_on_device({k: t for k, t in [(label, pts_t)] + [(f"out[{k!r}]", t) for k, t in list(out.items()) + list(side_out.items())] if hasattr(t, "device")})
        for name in names:
            if name not in out:
                import torch
                _, dt, k = QUERY_CHANNELS[name]
                out[name] = torch.empty((n, k) if k > 1 else (n,), dtype=torch.float32 if dt == np.float32 else torch.int32, device=pts_t.device)
                setattr(buf, name, out[name].data_ptr())
        for name, dt in side.items():
            if name not in side_out:
                import torch
                side_out[name] = torch.empty((n,), dtype=torch.float32 if dt == np.float32 else torch.int32, device=pts_t.device)
                side_ptr[name] = side_out[name].data_ptr()
        bits = sum(QUERY_CHANNELS[name][0] for name in names)

        def launch():
            if signed is not None:
                self._chk(self.lib.rtx_query_signed_distance(self.ctx, ptr, n, bits, C.byref(buf), side_ptr["signed_distance"], side_ptr.get("feature"), fl,
                                                             None if filt is None else C.byref(filt)), "rtx_query_signed_distance")
            elif filt is None:
                self._chk(getattr(self.lib, fn)(self.ctx, ptr, n, bits, C.byref(buf), fl), fn)
            else:
                self._chk(getattr(self.lib, fn + "_filtered")(self.ctx, ptr, n, bits, C.byref(buf), fl, C.byref(filt)), fn + "_filtered")
        tensors = [t for t in [pts_t, mask_t] + list(out.values()) + list(side_out.values()) if hasattr(t, "record_stream")]
        if tensors:
            self._on_torch_stream(launch, tensors)
        else:
            launch()
        return {**{name: side_out[name] for name in side}, **{name: out[name] for name in names}}

    def query_sweep(self, sweeps, channels=("distance",), out: Optional[Dict] = None, n: Optional[int] = None, sort: bool = False, mask=None) -> Dict:
        """The first contact of n moving balls with the frame the context holds (rtx_query_sweep): sweeps = float32 torch tensor (n, 8) of
        (origin, direction, max distance D, radius r) on this context's GPU; channels as for query_closest.  The centre moves along
        origin + t * direction; "distance" is the smallest t in [0, D) at which the ball touches the surface query_nearest measures (0 when
        it touches at its origin), "position" the contact point on the surface, normal, uv and ids what query_nearest reports for that
        point; the geometric contact normal is (origin + t * direction - position) / r.  No answer (nothing touched before D, a zero
        direction, a non-finite component, D or r NaN or not above 0, r infinite): distance inf, ids -1, the rest 0; +inf is a legal D.
        r and distances are measured in each instance's local space (rigid poses only, as for query_nearest).  Queued on torch's current stream, checked and shaped like
        query_nearest; sort=True (RTX_QUERY_SORT) walks the rows of every round in the ray queries' order, same answers row for row.
        Raw device pointers: sweeps = address, n, out = {name: address} for every channel wanted.  mask: as for query_nearest — hidden
        objects neither stop the ball nor overlap it."""
        return self._query_rows_to_channels("rtx_query_sweep", "sweeps", sweeps, 8, channels, out, n, sort, mask)

    def query_hits(self, segments, max_hits: int = 4, channels=("distance",), count: bool = True, out: Optional[Dict] = None, n: Optional[int] = None,
                   sort: bool = False, mask=None) -> Dict:
        """Every hit along n segments against the frame the context holds (rtx_query_hits): segments = float32 torch tensor (n, 7) of (origin,
        direction, max distance) on this context's GPU, the rows of query_occluded.  Returns {name: tensor} of the nearest max_hits hits of
        every row in ascending order — (n, K), (n, K, 3) or (n, K, 2), K = max_hits in [1, 8], channels as for query_closest — plus "count",
        the int32 tensor (n,) of the row's hits (it may exceed K), unless count=False.  Entries past min(count, K): distance inf, ids -1, the
        rest 0.  A sphere counts at both crossings; a dead row (zero direction, a non-finite component, a max distance that is NaN or not above
        0) has count 0.  max_hits=0 with channels=() returns the count only.  out = {name: tensor} supplies the tensors ("count" included).
        Queued on torch's current stream, checked like query_nearest; sort=True (RTX_QUERY_SORT): same answers row for row.  Raw device
        pointers: segments = address, n, out = {name: address} for every channel wanted and for "count" if count.  mask: as for
        query_nearest — hidden objects are neither listed nor counted; max_hits=1 is the filtered closest hit, the count-only form the
        filtered occlusion test."""
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
            raise TypeError(f"max_hits must be an int, not {type(max_hits).__name__}")
        K = int(max_hits)
        if not 0 <= K <= RTX_QUERY_MAX_HITS:
            raise ValueError(f"max_hits must be in [0, {RTX_QUERY_MAX_HITS}], not {K}")
        empty = not isinstance(channels, (str, int, np.integer)) and len(tuple(channels)) == 0 or (isinstance(channels, (int, np.integer)) and not isinstance(channels, bool) and int(channels) == 0)
        if K == 0:
            if not empty:
                raise ValueError("max_hits=0 is the count-only form: channels must be ()")
            if not count:
                raise ValueError("max_hits=0 is the count-only form: count must be True")
            names = ()
        else:
            names = query_names(channels)
        ptr, n, seg_t = self._query_rows("segments", segments, 7, n)
        if out is not None and not isinstance(out, dict):
            raise TypeError(f"out must be a dict {{channel name: tensor}}, not {type(out).__name__}")
        out = dict(out or {})
        wanted = names + (("count",) if count else ())
        for k in out:
            if k != "count":
                query_names((k,))
        extra = [k for k in out if k not in wanted]
        if extra:
            raise ValueError(f"out holds channels that were not requested: {', '.join(extra)}")
        raw = seg_t is None
        if raw and len(out) != len(wanted):
            raise ValueError("with raw device pointers out must hold an address for every requested channel and for the count")
        fl = RTX_QUERY_SORT if sort else 0
        filt, mask_t = self._query_filter(mask, n)
        buf = RtxQueryBuffers()
        cptr = None
        for name in out:
            if name == "count":
                cptr = self._query_out("count", out[name], np.int32, n, 1, raw)
            else:
                _, dt, k = QUERY_CHANNELS[name]
                setattr(buf, name, self._query_out(name, out[name], dt, n, k, raw, K))
        self._query_on_device({k: t for k, t in [("segments", seg_t)] + [(f"out[{k!r}]", t) for k, t in out.items()] if hasattr(t, "device")})
        for name in wanted:
            if name not in out:
                import torch
                if name == "count":
                    out[name] = torch.empty((n,), dtype=torch.int32, device=seg_t.device)
                    cptr = out[name].data_ptr()
                else:
                    _, dt, k = QUERY_CHANNELS[name]
                    out[name] = torch.empty(self._query_shape(n, k, K), dtype=torch.float32 if dt == np.float32 else torch.int32, device=seg_t.device)
                    setattr(buf, name, out[name].data_ptr())
        bits = sum(QUERY_CHANNELS[name][0] for name in names)

        def launch():
            if filt is None:
                self._chk(self.lib.rtx_query_hits(self.ctx, ptr, n, K, bits, C.byref(buf), cptr, fl), "rtx_query_hits")
            else:
                self._chk(self.lib.rtx_query_hits_filtered(self.ctx, ptr, n, K, bits, C.byref(buf), cptr, fl, C.byref(filt)), "rtx_query_hits_filtered")
        tensors = [t for t in [seg_t, mask_t] + list(out.values()) if hasattr(t, "record_stream")]
        if tensors:
            self._on_torch_stream(launch, tensors)
        else:
            launch()
        return {name: out[name] for name in wanted}

    def _query_overlap(self, boxes, K: int, count: bool, flags: int, out: Optional[Dict], n: Optional[int], sort: bool, mask, wanted: tuple,
                       rows: str = "boxes", width: int = 10, call: str = "rtx_query_overlap") -> Dict:
        """query_overlap and query_overlapped (and their capsule forms: rows, width, call): rows of `width` floats in, the int32 tensors named
        in `wanted` out."""
        ptr, n, box_t = self._query_rows(rows, boxes, width, n)
        if out is not None and not isinstance(out, dict):
            raise TypeError(f"out must be a dict {{name: tensor}}, not {type(out).__name__}")
        out = dict(out or {})
        extra = [k for k in out if k not in wanted]
        if extra:
            raise ValueError(f"out holds outputs that were not requested: {', '.join(map(str, extra))}")
        raw = box_t is None
        if raw and len(out) != len(wanted):
            raise ValueError("with raw device pointers out must hold an address for every output: " + ", ".join(wanted))
        fl = flags | (RTX_QUERY_SORT if sort else 0)
        filt, mask_t = self._query_filter(mask, n)
        ptrs = {name: self._query_out(name, t, np.int32, n, 1, raw, 0 if name == "count" else K) for name, t in out.items()}
        self._query_on_device({k: t for k, t in [(rows, box_t)] + [(f"out[{k!r}]", t) for k, t in out.items()] if hasattr(t, "device")})
        for name in wanted:
            if name not in out:
                import torch
                out[name] = torch.empty((n,) if name == "count" else (n, K), dtype=torch.int32, device=box_t.device)
                ptrs[name] = out[name].data_ptr()

        def launch():
            args = (self.ctx, ptr, n, K, ptrs.get("object_id"), ptrs.get("triangle_id"), ptrs.get("count"), fl)
            if filt is None:
                self._chk(getattr(self.lib, call)(*args), call)
            else:
                self._chk(getattr(self.lib, call + "_filtered")(*args, C.byref(filt)), call + "_filtered")
        tensors = [t for t in [box_t, mask_t] + list(out.values()) if hasattr(t, "record_stream")]
        if tensors:
            self._on_torch_stream(launch, tensors)
        else:
            launch()
        return {name: out[name] for name in wanted}

    def query_overlap(self, boxes, max_hits: int = 4, count: bool = True, objects: bool = False, out: Optional[Dict] = None, n: Optional[int] = None,
                      sort: bool = False, mask=None) -> Dict:
        """What n oriented boxes touch in the frame the context holds (rtx_query_overlap): boxes = float32 torch tensor (n, 10) of (centre,
        half extents, rotation quaternion x y z w — update_instances' convention, normalised by the library) on this context's GPU.  Returns
        {"object_id": (n, K), "triangle_id": (n, K), "count": (n,)} int32, K = max_hits in [1, 8]: the K smallest (object, triangle slot)
        overlaps of every row in ascending order, entries past the count -1, triangle_id -1 for spheres and planes; "count" (unless
        count=False) is the number of all overlaps and may exceed K.  objects=True (RTX_OVERLAP_OBJECTS): the distinct objects — an instance
        counts once — and no "triangle_id".  max_hits=0 gives the count alone.  A triangle overlaps when the box touches it (touching
        counts), a sphere when its shell meets the box, a plane when the box reaches it; a dead row (a non-finite float, a negative half
        extent, a zero quaternion) overlaps nothing; zero half extents are fine.  out = {name: tensor} supplies the tensors.  Queued on
        torch's current stream, checked like query_nearest; sort=True (RTX_QUERY_SORT): the rows are walked in the Morton order of their
        centres, same answers row for row.  Raw device pointers: boxes = address, n, out = {name: address} for every output.  mask: as for
        query_nearest — hidden objects are neither listed nor counted."""
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
            raise TypeError(f"max_hits must be an int, not {type(max_hits).__name__}")
        K = int(max_hits)
        if not 0 <= K <= RTX_QUERY_MAX_HITS:
            raise ValueError(f"max_hits must be in [0, {RTX_QUERY_MAX_HITS}], not {K}")
        if K == 0 and not count:
            raise ValueError("max_hits=0 is the count-only form: count must be True")
        wanted = (("object_id",) + (() if objects else ("triangle_id",)) if K else ()) + (("count",) if count else ())
        return self._query_overlap(boxes, K, bool(count), RTX_OVERLAP_OBJECTS if objects else 0, out, n, sort, mask, wanted)

    def query_overlapped(self, boxes, out=None, n: Optional[int] = None, sort: bool = False, mask=None):
        """Whether each of n oriented boxes touches anything (rtx_query_overlap with RTX_OVERLAP_ANY): the int32 tensor (n,) of 1 / 0 (out,
        or a new one) — the sibling of query_occluded; a row's walk ends at its first overlap.  boxes, sort, mask, raw pointers and checks
        as for query_overlap; grid_boxes() makes the rows of a voxel grid."""
        if out is None and isinstance(boxes, (int, np.integer)) and not isinstance(boxes, bool):
            raise ValueError("with raw device pointers out must be the address of the result")
        return self._query_overlap(boxes, 0, True, RTX_OVERLAP_ANY, None if out is None else {"count": out}, n, sort, mask, ("count",))["count"]

    def query_overlap_capsule(self, capsules, max_hits: int = 4, count: bool = True, objects: bool = False, out: Optional[Dict] = None, n: Optional[int] = None,
                              sort: bool = False, mask=None) -> Dict:
        """What n capsules touch in the frame the context holds (rtx_query_overlap_capsule): capsules = float32 torch tensor (n, 7) of (start
        point p, axis vector d, radius r) on this context's GPU — every point within r of the segment p + s d, s in [0, 1]; d = 0 is a ball
        (every primitive within r of p), r = 0 a segment; capsule_rows() makes the rows from end points.  The outputs, max_hits, count,
        objects, out, raw pointers, mask and checks are query_overlap's.  A triangle overlaps when its distance to the segment is <= r
        (touching counts), a sphere when its shell meets the capsule, a plane when the capsule reaches it; a dead row (a non-finite float, a
        negative radius) overlaps nothing.  sort=True (RTX_QUERY_SORT): the rows are walked in the order of the ray key over (p, d), same
        answers row for row; ball rows have no ray key and are walked last."""
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
            raise TypeError(f"max_hits must be an int, not {type(max_hits).__name__}")
        K = int(max_hits)
        if not 0 <= K <= RTX_QUERY_MAX_HITS:
            raise ValueError(f"max_hits must be in [0, {RTX_QUERY_MAX_HITS}], not {K}")
        if K == 0 and not count:
            raise ValueError("max_hits=0 is the count-only form: count must be True")
        wanted = (("object_id",) + (() if objects else ("triangle_id",)) if K else ()) + (("count",) if count else ())
        return self._query_overlap(capsules, K, bool(count), RTX_OVERLAP_OBJECTS if objects else 0, out, n, sort, mask, wanted,
                                   "capsules", 7, "rtx_query_overlap_capsule")

    def query_overlapped_capsule(self, capsules, out=None, n: Optional[int] = None, sort: bool = False, mask=None):
        """Whether each of n capsules touches anything (rtx_query_overlap_capsule with RTX_OVERLAP_ANY): the int32 tensor (n,) of 1 / 0 (out,
        or a new one); a row's walk ends at its first overlap.  capsules, sort, mask, raw pointers and checks as for query_overlap_capsule."""
        if out is None and isinstance(capsules, (int, np.integer)) and not isinstance(capsules, bool):
            raise ValueError("with raw device pointers out must be the address of the result")
        return self._query_overlap(capsules, 0, True, RTX_OVERLAP_ANY, None if out is None else {"count": out}, n, sort, mask, ("count",),
                                   "capsules", 7, "rtx_query_overlap_capsule")["count"]

    # the outputs of query_sweep_box, in the order of rtx_query_sweep_box's arguments: name -> (dtype, width)
    SWEEP_BOX_OUTPUTS = {"distance": (np.float32, 1), "normal": (np.float32, 3), "object_id": (np.int32, 1), "triangle_id": (np.int32, 1), "axis": (np.int32, 1)}

    def query_sweep_box(self, sweeps, channels=("distance",), out: Optional[Dict] = None, n: Optional[int] = None, sort: bool = False, mask=None) -> Dict:
        """The first contact of n moving oriented boxes with the frame the context holds (rtx_query_sweep_box): sweeps = float32 torch tensor
        (n, 14) of (centre, direction, max distance D, half extents, rotation quaternion x y z w — query_overlap's box) on this context's GPU;
        channels = names out of distance, normal, object_id, triangle_id, axis.  The centre moves along centre + t * direction without
        turning; "distance" is the smallest t in [0, D) at which the box touches a triangle, a sphere's shell or a plane (0 when it touches
        where it starts), "normal" the unit contact normal opposing the motion (0 at t == 0), "axis" the contact's kind: 0..2 a box face,
        3 the triangle's face, 4..12 edge against edge (box axis (k - 4) % 3, triangle edge (k - 4) // 3), 13 an overlap at t == 0,
        14 a sphere, 15 a plane.  No answer (nothing touched before D, or a dead row: a zero direction, a non-finite float, D NaN or not
        above 0, a negative half extent, a zero quaternion): distance inf, ids and axis -1, normal 0; +inf is a legal D, zero half extents
        are fine.  Returns {name: tensor}: float32 / int32, (n,) or (n, 3), allocated on the device unless out = {name: tensor} supplies them.
        Queued on torch's current stream, checked like query_nearest; sort=True (RTX_QUERY_SORT) walks the rows of every round in the ray
        queries' order, same answers row for row.  Raw device pointers: sweeps = address, n, out = {name: address} for every channel wanted.
        mask: as for query_nearest — hidden objects neither stop the box nor overlap it."""
        if isinstance(channels, str):
            channels = (channels,)
        names = tuple(channels)
        if not names:
            raise ValueError("channels must name at least one of " + ", ".join(self.SWEEP_BOX_OUTPUTS))
        for name in names:
            if name not in self.SWEEP_BOX_OUTPUTS:
                raise ValueError(f"unknown channel {name!r}: query_sweep_box has " + ", ".join(self.SWEEP_BOX_OUTPUTS))
        if len(set(names)) != len(names):
            raise ValueError("channels names a channel twice")
        ptr, n, rows_t = self._query_rows("sweeps", sweeps, 14, n)
        if out is not None and not isinstance(out, dict):
            raise TypeError(f"out must be a dict {{channel name: tensor}}, not {type(out).__name__}")
        out = dict(out or {})
        extra = [k for k in out if k not in names]
        if extra:
            raise ValueError(f"out holds channels that were not requested: {', '.join(map(str, extra))}")
        raw = rows_t is None
        if raw and len(out) != len(names):
            raise ValueError("with raw device pointers out must hold an address for every requested channel")
        fl = RTX_QUERY_SORT if sort else 0
        filt, mask_t = self._query_filter(mask, n)
        ptrs = {name: self._query_out(name, t, self.SWEEP_BOX_OUTPUTS[name][0], n, self.SWEEP_BOX_OUTPUTS[name][1], raw) for name, t in out.items()}
        self._query_on_device({k: t for k, t in [("sweeps", rows_t)] + [(f"out[{k!r}]", t) for k, t in out.items()] if hasattr(t, "device")})
        for name in names:
            if name not in out:
                import torch
                dt, k = self.SWEEP_BOX_OUTPUTS[name]
                out[name] = torch.empty(self._query_shape(n, k), dtype=torch.float32 if dt == np.float32 else torch.int32, device=rows_t.device)
                ptrs[name] = out[name].data_ptr()

        def launch():
            args = (self.ctx, ptr, n, ptrs.get("distance"), ptrs.get("normal"), ptrs.get("object_id"), ptrs.get("triangle_id"), ptrs.get("axis"), fl)
            if filt is None:
                self._chk(self.lib.rtx_query_sweep_box(*args), "rtx_query_sweep_box")
            else:
                self._chk(self.lib.rtx_query_sweep_box_filtered(*args, C.byref(filt)), "rtx_query_sweep_box_filtered")
        tensors = [t for t in [rows_t, mask_t] + list(out.values()) if hasattr(t, "record_stream")]
        if tensors:
            self._on_torch_stream(launch, tensors)
        else:
            launch()
        return {name: out[name] for name in names}

    def debug_query_order(self, rows, n: Optional[int] = None):
        """The order sort=True traces the rows in (rtx_debug_query_order): rows = float32 torch tensor (n, 6) of rays, (n, 7) of segments or (n, 4) of
        query_nearest points on this context's GPU; returns the int32 tensor (n,): element first + i = the row traced in slot i of the round that starts at row
        `first`.  Nothing is traced.  Queued on torch's current stream like the queries."""
        import torch
        width = rows.shape[1] if isinstance(rows, torch.Tensor) and rows.dim() == 2 else 0
        if width not in (4, 6, 7):
            raise ValueError(f"rows must have shape (n, 4), (n, 6) or (n, 7), not {tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__}")
        ptr, n, rows_t = self._query_rows("rows", rows, width, n)
        self._query_on_device({"rows": rows_t})
        out = torch.empty((n,), dtype=torch.int32, device=rows_t.device)
        optr = out.data_ptr()

        def launch():
            self._chk(self.lib.rtx_debug_query_order(self.ctx, ptr, width, n, optr), "rtx_debug_query_order")
        self._on_torch_stream(launch, [rows_t, out])
        return out

    def enable_timing(self, on: bool = True):
        self._chk(self.lib.rtx_enable_kernel_timing(self.ctx, 1 if on else 0), "rtx_enable_kernel_timing")

    def kernel_times(self):
        cap = 65536
        names = (C.c_char_p * cap)(); ms = (C.c_float * cap)(); n = C.c_int32()
        self._chk(self.lib.rtx_last_kernel_times(self.ctx, names, ms, cap, C.byref(n)), "rtx_last_kernel_times")
        return [(names[i].decode(), float(ms[i])) for i in range(min(n.value, cap))]

    # ---- GPU groups (include/rtx.h: rtx_group_*) ----------------------------------------------------------------
    @staticmethod
    def group_unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.rtx_group_unique_id(buf)
        if rc:
            raise RtxError(rc, "rtx_group_unique_id")
        return buf.raw

    def group_create(self, rank: int, world: int, unique_id: Optional[bytes] = None):
        self.group = C.c_void_p()
        self._chk(self.lib.rtx_group_create(self.ctx, rank, world, unique_id, C.byref(self.group)), "rtx_group_create")

    def group_attach(self, base: "Renderer"):
        """Another frame in flight on the same GPU: joins `base`'s communicator as the same rank (rtx_group_attach)."""
        self.group = C.c_void_p()
        self._chk(self.lib.rtx_group_attach(self.ctx, base.group, C.byref(self.group)), "rtx_group_attach")

    def group_render(self, cull_dead_shadow_rays: bool = False, lane_trace: bool = False):
        flags = (RTX_RENDER_CULL_DEAD_SHADOW_RAYS if cull_dead_shadow_rays else 0) | (RTX_RENDER_LANE_TRACE if lane_trace else 0)
        self._chk(self.lib.rtx_group_render(self.group, flags), "rtx_group_render")

    def group_destroy(self):
        if getattr(self, "group", None):
            self.lib.rtx_group_destroy(self.group); self.group = None

    def group_loopback(self, world: int, flags: int = 0):
        self._chk(self.lib.rtx_debug_group_loopback(self.ctx, world, flags), "rtx_debug_group_loopback")

    # ---- unit-level hooks ---------------------------------------------------------------------------
    def debug_libm(self, fn: int, a: np.ndarray, b: Optional[np.ndarray] = None) -> np.ndarray:
        """rtx_debug_libm: fn 0 acosf 1 atan2f(a, b) 2 expf 3 log2f 4 atanf 5 f2i_rn_x86 6 1 / sqrtf 7 f2i_trunc_x86 8 pow2_128, as the device
        build computes them; 5 and 7 come back as floats.  Any other id raises RtxError (RTX_ERR_INVALID_ARG)."""
        a = np.ascontiguousarray(a, np.float32)
        bb = np.ascontiguousarray(b, np.float32) if b is not None else a
        out = np.zeros_like(a)
        self._chk(self.lib.rtx_debug_libm(self.ctx, fn, a.ctypes.data, bb.ctypes.data, out.ctypes.data, a.size), "rtx_debug_libm")
        return out

    def debug_texture_sample(self, texture_id: int, in6: np.ndarray) -> np.ndarray:
        in6 = np.ascontiguousarray(in6, np.float32)
        out = np.zeros((in6.shape[0], 3), np.float32)
        self._chk(self.lib.rtx_debug_texture_sample(self.ctx, texture_id, in6.ctypes.data, out.ctypes.data, in6.shape[0]), "rtx_debug_texture_sample")
        return out

    def debug_trace_rays(self, rays18: np.ndarray, flags: int = 0) -> np.ndarray:
        rays18 = np.ascontiguousarray(rays18, np.float32)
        out = np.zeros((rays18.shape[0], 27), np.float32)
        self._chk(self.lib.rtx_debug_trace_rays(self.ctx, rays18.ctypes.data, rays18.shape[0], out.ctypes.data, flags), "rtx_debug_trace_rays")
        return out

    def debug_blas_wide(self, blas_id: int) -> int:
        need = C.c_int32(0)
        self._chk(self.lib.rtx_debug_blas_wide(self.ctx, blas_id, C.byref(need)), "rtx_debug_blas_wide")
        return int(need.value)

    def debug_blas_wide_closest(self, blas_id: int) -> int:
        need = C.c_int32(0)
        self._chk(self.lib.rtx_debug_blas_wide_closest(self.ctx, blas_id, C.byref(need)), "rtx_debug_blas_wide_closest")
        return int(need.value)

    def debug_occluded(self, origin_direction_maxdist7: np.ndarray, flags: int = 0) -> np.ndarray:
        r = np.ascontiguousarray(origin_direction_maxdist7, np.float32)
        out = np.zeros(r.shape[0], np.uint32)
        self._chk(self.lib.rtx_debug_occluded(self.ctx, r.ctypes.data, r.shape[0], out.ctypes.data, flags), "rtx_debug_occluded")
        return out

    def debug_light_plot(self, pl, sl, dl, in10: np.ndarray, rgb: np.ndarray):
        in10 = np.ascontiguousarray(in10, np.float32); rgb = np.ascontiguousarray(rgb, np.float32)
        out9 = np.zeros((in10.shape[0], 9), np.float32); packed = np.zeros(rgb.shape[0], np.uint32)
        self._chk(self.lib.rtx_debug_light_plot(self.ctx, pl.ctypes.data, sl.ctypes.data, dl.ctypes.data, in10.ctypes.data, out9.ctypes.data, in10.shape[0],
                                                rgb.ctypes.data, packed.ctypes.data, rgb.shape[0]), "rtx_debug_light_plot")
        return out9, packed

    def debug_sky_sample(self, dirs: np.ndarray) -> np.ndarray:
        dirs = np.ascontiguousarray(dirs, np.float32)
        out = np.zeros_like(dirs)
        self._chk(self.lib.rtx_debug_sky_sample(self.ctx, dirs.ctypes.data, out.ctypes.data, dirs.shape[0]), "rtx_debug_sky_sample")
        return out
