"""Per-pixel primary-hit AOVs (include/rtx.h rtx_bind_aovs / rtx_read_aovs, RTX_RENDER_AOV): the declarations, exported symbols and
ctypes mirrors, and the Python-side argument checks, without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest

from util import REPO


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    return a


NEW = ("rtx_bind_aovs", "rtx_read_aovs")
HEADER_CHANNELS = ("DEPTH", "POSITION", "NORMAL", "ALBEDO", "UV", "MATERIAL_ID", "OBJECT_ID", "TRIANGLE_ID")


def _header():
    return open(f"{REPO}/include/rtx.h").read()


def test_aov_functions_are_declared_exported_and_bound(api):
    header = _header()
    lib = api.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in api.EXPORTS, name
        assert getattr(lib, name).argtypes, name
    assert re.search(r"RTX_RENDER_AOV\s*=\s*128\b", header) and api.RTX_RENDER_AOV == 128
    assert api.render_flags(aov=True) == 128 and api.render_flags(serial=True, aov=True) == 128 | api.RTX_RENDER_SERIAL


def test_aov_bits_and_struct_layout_match_the_header(api):
    from pyrtx import ctypes_structs as cs
    header = _header()
    for k, name in enumerate(HEADER_CHANNELS):
        m = re.search(r"\bRTX_AOV_" + name + r"\s*=\s*(\d+)", header)
        assert m and int(m.group(1)) == 1 << k, name
        assert getattr(cs, "RTX_AOV_" + name) == 1 << k
        assert cs.AOV_CHANNELS[name.lower()][0] == 1 << k
    assert int(re.search(r"\bRTX_AOV_ALL\s*=\s*(\d+)", header).group(1)) == cs.RTX_AOV_ALL == 255
    # rtx_aov_buffers: eight pointers in channel-bit order, the same names as the Python channels
    body = re.search(r"typedef struct rtx_aov_buffers \{(.*?)\} rtx_aov_buffers;", header, re.S).group(1)
    fields = re.findall(r"\b(?:float|int32_t)\s*\*\s*(\w+);", body)
    assert fields == [n.lower() for n in HEADER_CHANNELS] == list(cs.AOV_CHANNELS)
    assert [f for f, _ in cs.RtxAovBuffers._fields_] == fields
    assert C.sizeof(cs.RtxAovBuffers) == 8 * C.sizeof(C.c_void_p)
    for k, (f, _) in enumerate(cs.RtxAovBuffers._fields_):
        assert getattr(cs.RtxAovBuffers, f).offset == 8 * k
    kinds = re.findall(r"\b(float|int32_t)\s*\*\s*\w+;", body)
    assert [np.float32 if t == "float" else np.int32 for t in kinds] == [cs.AOV_CHANNELS[f][1] for f in fields]


def test_aov_names_and_masks(api):
    assert api.aov_mask("depth") == 1 and api.aov_mask(["uv", "depth"]) == 17
    assert api.aov_names(["uv", "depth", "uv"]) == ("depth", "uv")          # channel order, duplicates folded
    assert api.aov_names(255) == ("depth", "position", "normal", "albedo", "uv", "material_id", "object_id", "triangle_id")
    assert api.aov_mask(()) == 0
    assert api.aov_shape("normal", 2, 70, 100) == (2, 70, 100, 3) and api.aov_shape("uv", None, 70, 100) == (70, 100, 2)
    assert api.aov_shape("object_id", 3, 70, 100) == (3, 70, 100)
    with pytest.raises(ValueError):
        api.aov_names(["depth", "z"])
    with pytest.raises(TypeError):
        api.aov_names([1, 2])
    with pytest.raises(ValueError):
        api.aov_names(256)


def _offline_renderer(api, width=64, height=48):
    """A Renderer object whose context was never created: any call that reached the library would fail on the None handles."""
    from pyrtx import scene_io as sio
    r = object.__new__(api.Renderer)
    sc = sio.Scene()
    sc.config["width"] = width; sc.config["height"] = height
    r.scene, r.device, r.ctx, r.lib = sc, 0, None, None
    return r


def test_aov_methods_validate_before_the_library(api):
    r = _offline_renderer(api)
    with pytest.raises(ValueError):
        r.render_aovs(channels=("depth", "colour"))
    with pytest.raises(ValueError):
        r.render_aovs(channels=())
    with pytest.raises(ValueError):
        r.bind_aovs(["depth"], {"depht": 0x1000}, 16)
    with pytest.raises(TypeError):
        r.read_aovs([0])
    with pytest.raises(ValueError):
        r.render_views(aovs=("normals",))


def test_render_views_into_validates_aovs_before_the_library(api):
    torch = pytest.importorskip("torch")
    r = _offline_renderer(api, 64, 48)
    rgb = torch.zeros((2, 48, 64, 3), dtype=torch.float32)
    packed = torch.zeros((2, 48, 64), dtype=torch.int32)
    depth = torch.zeros((2, 48, 64), dtype=torch.float32)
    cases = [
        ({"depth": depth.numpy()}, TypeError, "torch.Tensor"),                                       # not a tensor
        ({"depth": depth.double()}, TypeError, "float32"),                                           # dtype
        ({"object_id": depth}, TypeError, "int32"),                                                  # ids are int32
        ({"normal": torch.zeros((2, 48, 64), dtype=torch.float32)}, ValueError, "shape"),            # (C, H, W, 3)
        ({"uv": torch.zeros((2, 48, 64, 3), dtype=torch.float32)}, ValueError, "shape"),             # (C, H, W, 2)
        ({"depth": torch.zeros((2, 64, 48), dtype=torch.float32)}, ValueError, "shape"),
        ({"depth": torch.zeros((3, 48, 64), dtype=torch.float32)}, ValueError, "numbers of views"),  # other view count than rgb
        ({"dpeth": depth}, ValueError, "unknown AOV channel"),
        ({7: depth}, TypeError, "names"),
        ([("depth", depth)], TypeError, "dict"),
        ({"depth": torch.zeros((2, 48, 128), dtype=torch.float32)[..., ::2]}, ValueError, "contiguous"),
        ({"depth": depth}, ValueError, "cuda:0"),                                                    # device: host tensors
    ]
    for aovs, exc, match in cases:
        with pytest.raises(exc, match=match):
            r.render_views_into(rgb, packed, 0, 1, aovs=aovs)
