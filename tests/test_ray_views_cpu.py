"""Ray views (include/rtx.h rtx_set_rays / rtx_bind_rays / rtx_render_rays): the exported symbols, pinhole_rays against the oracle and the
Python-side argument checks, without a GPU."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import util
from util import REPO
from test_views_cpu import _offline_renderer

f32 = np.float32
NEW = ("rtx_set_rays", "rtx_bind_rays", "rtx_render_rays")


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    return a


def test_ray_functions_are_declared_exported_and_bound(api):
    from pyrtx import ctypes_structs as cs
    header = open(f"{REPO}/include/rtx.h").read()
    assert re.search(r"#define\s+RTX_ABI_VERSION\s+1\b", header)
    m = re.search(r"typedef\s+struct\s+rtx_ray\s*\{(.*?)\}\s*rtx_ray\s*;", header, re.S)
    assert m, "rtx_ray is not declared"
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = re.findall(r"(\w+)\s*\[\s*3\s*\]", fields)
    assert names == ["origin", "direction", "dO_dx", "dO_dy", "dD_dx", "dD_dy"] and re.match(r"\s*float\b", fields)
    assert [n for n, _ in cs.RtxRay._fields_] == names and C.sizeof(cs.RtxRay) == 72 and api.RAY_FLOATS == 18
    lib = api.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"\sT\s+" + name + r"\b", exported), f"{name} is not exported by the library"
        assert name in api.EXPORTS, name
        assert getattr(lib, name).argtypes, name
        assert getattr(lib, name).restype is C.c_int, name
    # the C side's sizeof(rtx_ray): the header's struct compiled by the host compiler
    src = f'#include "{REPO}/include/rtx.h"\n#include <stdio.h>\nint main(void) {{ printf("%zu", sizeof(rtx_ray)); return 0; }}\n'
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["cc", "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
        assert subprocess.run([os.path.join(d, "s")], capture_output=True, text=True, check=True).stdout == "72"


def _scene(name):
    if name == "ragged":                       # 100x70: edge tiles clipped in both directions
        sc, _ = util.load_golden("materials_aniso")
        sc.config["width"] = 100; sc.config["height"] = 70
        return sc
    return util.load_golden(name)[0]


@pytest.mark.parametrize("name", ["cube", "materials_aniso", "camera_keys", "tori16", "ragged"])
def test_pinhole_rays_are_the_oracles_primary_rays(api, name):
    """orc_trace_closest of pinhole_rays finds, for EVERY pixel, exactly the distance the oracle's own render reports for its primary ray
    (inf on a miss): origin and direction are the oracle's.  camera_keys has a rotated camera."""
    import orc
    sc = _scene(name)
    rays = api.pinhole_rays(sc.camera[0], sc.width, sc.height)
    assert rays.shape == (sc.height, sc.width, 18) and rays.dtype == f32 and rays.flags.c_contiguous
    assert not rays[..., 6:12].any(), "origin differentials of a pinhole camera are zero"
    assert (rays[..., 0:3] == np.asarray(sc.camera[0]["position"], f32)).all()
    o = orc.OracleScene(sc)
    dist = o.render(threads=8, want_dist=True)["dist"].reshape(-1)
    hits, _ = o.trace_closest(rays.reshape(-1, 18), 8)
    a, b = np.ascontiguousarray(hits[:, 1], f32).view(np.uint32), np.ascontiguousarray(dist, f32).view(np.uint32)
    assert a.shape == b.shape and (a == b).all(), f"{int((a != b).sum())} of {a.size} pixels differ"
    assert (hits[:, 0] > 0).any() and np.isfinite(dist).any()
    # 12 floats and a CAMERA record are the same camera
    row = np.concatenate([np.asarray(sc.camera[0][k], f32) for k in ("position", "rotated_top_left_corner", "rotated_x_axis", "rotated_y_axis")])
    assert api.pinhole_rays(row, sc.width, sc.height).tobytes() == rays.tobytes()


def test_rays_from_directions_differences():
    from pyrtx import api
    rng = np.random.default_rng(5)
    o = rng.normal(size=(4, 5, 3)).astype(f32); d = rng.normal(size=(4, 5, 3)).astype(f32)
    r = api.rays_from_directions(o, d)
    assert r.shape == (4, 5, 18) and r.dtype == f32
    assert np.array_equal(r[..., 0:3], o) and np.array_equal(r[..., 3:6], d)
    assert np.array_equal(r[:, :-1, 12:15], d[:, 1:] - d[:, :-1]) and np.array_equal(r[:, -1, 12:15], d[:, -1] - d[:, -2])      # forward, last column backward
    assert np.array_equal(r[:-1, :, 15:18], d[1:] - d[:-1]) and np.array_equal(r[-1, :, 15:18], d[-1] - d[-2])
    assert np.array_equal(r[:, :-1, 6:9], o[:, 1:] - o[:, :-1]) and np.array_equal(r[:-1, :, 9:12], o[1:] - o[:-1])
    one = api.rays_from_directions(o[:1, :1], d[:1, :1])
    assert not one[..., 6:].any()
    with pytest.raises(ValueError):
        api.rays_from_directions(o, d[:, :4])


def test_rays_array_accepts_one_view_and_batches(api):
    r = np.arange(48 * 64 * 18, dtype=f32).reshape(48, 64, 18)
    a = api.rays_array(r, 64, 48)
    assert a.shape == (1, 48, 64, 18) and a.tobytes() == r.tobytes()
    b = api.rays_array(np.stack([r, r])[:, :, :, :], 64, 48)
    assert b.shape == (2, 48, 64, 18) and b.flags.c_contiguous


@pytest.mark.parametrize("bad,exc", [
    (lambda: np.zeros((2, 48, 64, 18), np.float64), TypeError),                 # dtype
    (lambda: np.zeros((2, 48, 64, 18), np.int32), TypeError),
    (lambda: [[0.0] * 18], TypeError),                                           # not an array
    (lambda: np.zeros((48 * 64, 18), f32), ValueError),                          # rank
    (lambda: np.zeros((1, 2, 48, 64, 18), f32), ValueError),
    (lambda: np.zeros((2, 48, 64, 17), f32), ValueError),                        # last dimension
    (lambda: np.zeros((48, 64, 6), f32), ValueError),
    (lambda: np.zeros((2, 64, 48, 18), f32), ValueError),                        # H / W not the context's
    (lambda: np.zeros((2, 48, 63, 18), f32), ValueError),
    (lambda: np.zeros((0, 48, 64, 18), f32), ValueError),                        # V = 0
    (lambda: np.broadcast_to(np.zeros((1, 48, 64, 18), f32), (4097, 48, 64, 18)), ValueError),      # V > RTX_MAX_VIEWS
])
def test_set_rays_validates_before_the_library(api, bad, exc):
    r = _offline_renderer(api, 64, 48)
    with pytest.raises(exc):
        r.set_rays(bad())


def test_render_rays_into_validates_before_the_library(api):
    torch = pytest.importorskip("torch")
    r = _offline_renderer(api, 64, 48)
    ok_rgb = torch.zeros((2, 48, 64, 3), dtype=torch.float32)
    ok_packed = torch.zeros((2, 48, 64), dtype=torch.int32)
    ok_rays = torch.zeros((2, 48, 64, 18), dtype=torch.float32)
    cases = [
        (ok_rgb, ok_packed, np.zeros((2, 48, 64, 18), f32), TypeError),                                   # not a tensor
        (ok_rgb, ok_packed, ok_rays.double(), TypeError),                                                # dtype
        (ok_rgb, ok_packed, ok_rays.int(), TypeError),
        (ok_rgb, ok_packed, torch.zeros((48, 64, 18), dtype=torch.float32), ValueError),                 # rank
        (ok_rgb, ok_packed, torch.zeros((2, 48, 64, 17), dtype=torch.float32), ValueError),              # last dimension
        (ok_rgb, ok_packed, torch.zeros((2, 64, 48, 18), dtype=torch.float32), ValueError),              # H / W
        (ok_rgb, ok_packed, torch.zeros((2, 48, 65, 18), dtype=torch.float32), ValueError),
        (ok_rgb, ok_packed, torch.zeros((0, 48, 64, 18), dtype=torch.float32), ValueError),              # V = 0
        (ok_rgb, ok_packed, torch.zeros((1, 48, 64, 18), dtype=torch.float32).expand(4097, 48, 64, 18), ValueError),      # V > 4096
        (ok_rgb, ok_packed, ok_rays, ValueError),                                                        # host tensors
        (ok_rgb.double(), ok_packed, ok_rays, (TypeError, ValueError)),
    ]
    for rgb, packed, rays, exc in cases:
        with pytest.raises(exc):
            r.render_rays_into(rgb, packed, rays)
    strided = torch.zeros((2, 48, 64, 36), dtype=torch.float32)[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        r.render_rays_into(ok_rgb, ok_packed, strided)
    with pytest.raises(ValueError, match="cuda:0"):
        r.render_rays_into(ok_rgb, ok_packed, ok_rays)
    with pytest.raises(ValueError, match="18"):
        r.render_rays_into(ok_rgb, ok_packed, torch.zeros((2, 48, 64, 3), dtype=torch.float32))
