"""Batches of camera views (include/rtx.h rtx_set_views ...): the exported symbols and the Python-side argument checks, without a GPU."""
import re

import numpy as np
import pytest

from util import REPO


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    return a


NEW = ("rtx_set_views", "rtx_render_views", "rtx_read_views", "rtx_bind_view_framebuffer")


def test_view_functions_are_declared_exported_and_bound(api):
    header = open(f"{REPO}/include/rtx.h").read()
    assert re.search(r"#define\s+RTX_MAX_VIEWS\s+4096\b", header) and api.RTX_MAX_VIEWS == 4096
    lib = api.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in api.EXPORTS, name
        assert getattr(lib, name).argtypes, name          # the binding declares its arguments


def test_views_array_accepts_camera_records_and_float_rows(api):
    from pyrtx import scene_io as sio
    rows = np.arange(3 * 12, dtype=np.float32).reshape(3, 12)
    cams = api.views_array(rows)
    assert cams.dtype == sio.CAMERA and cams.shape == (3,) and cams.tobytes() == rows.tobytes()
    again = api.views_array(cams)
    assert again.tobytes() == rows.tobytes()
    assert api.views_array(rows[::2]).tobytes() == rows[::2].tobytes()          # strided input is made contiguous


@pytest.mark.parametrize("bad,exc", [
    (np.zeros((3, 12), np.float64), TypeError),
    (np.zeros((3, 11), np.float32), ValueError),
    (np.zeros(12, np.float32), ValueError),
    (np.zeros((0, 12), np.float32), ValueError),
    (np.zeros((4097, 12), np.float32), ValueError),
    ([[0.0] * 12], TypeError),
])
def test_views_array_rejects_bad_cameras(api, bad, exc):
    with pytest.raises(exc):
        api.views_array(bad)


def _offline_renderer(api, width=64, height=48):
    """A Renderer object whose context was never created: any call that reached the library would fail on the None handles."""
    from pyrtx import scene_io as sio
    r = object.__new__(api.Renderer)
    sc = sio.Scene()
    sc.config["width"] = width; sc.config["height"] = height
    r.scene, r.device, r.ctx, r.lib = sc, 0, None, None
    return r


def test_set_views_validates_before_the_library(api):
    from pyrtx import scene_io as sio
    r = _offline_renderer(api)
    with pytest.raises(ValueError):
        r.set_views(np.zeros((2, 2), sio.CAMERA))
    with pytest.raises(TypeError):
        r.set_views(np.zeros((2, 12), np.int32))


def test_render_views_into_validates_before_the_library(api):
    torch = pytest.importorskip("torch")
    r = _offline_renderer(api, 64, 48)
    ok_rgb = torch.zeros((2, 48, 64, 3), dtype=torch.float32)
    ok_packed = torch.zeros((2, 48, 64), dtype=torch.int32)
    cases = [
        (np.zeros((2, 48, 64, 3), np.float32), ok_packed, TypeError),                   # not a tensor
        (ok_rgb.double(), ok_packed, TypeError),                                        # dtype
        (ok_rgb, ok_packed.float(), TypeError),
        (torch.zeros((2, 48, 64), dtype=torch.float32), ok_packed, ValueError),         # shape
        (torch.zeros((2, 64, 48, 3), dtype=torch.float32), ok_packed, ValueError),
        (ok_rgb, torch.zeros((2, 48, 63), dtype=torch.int32), ValueError),
        (ok_rgb, ok_packed, ValueError),                                                # device: host tensors
    ]
    for rgb, packed, exc in cases:
        with pytest.raises(exc):
            r.render_views_into(rgb, packed, 0, 1)
    strided = torch.zeros((2, 48, 64, 6), dtype=torch.float32)[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        r.render_views_into(strided, ok_packed, 0, 1)
    with pytest.raises(ValueError, match="cuda:0"):
        r.render_views_into(ok_rgb, ok_packed, 0, 1)
