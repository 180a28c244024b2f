"""Batches of camera views of one frame (include/rtx.h rtx_set_views / rtx_render_views / rtx_read_views / rtx_bind_view_framebuffer).

Every view of a rtx_render_views call must be BIT-EXACT (fp32 colour, packed pixel) against a single-view rtx_set_frame +
rtx_render_tiles render of its camera and against the oracle with that camera, and the call's ray counts must be the sum of the
single-view counts.  Camera sets hold the scene's own camera plus moved / rotated ones made by the host library's Camera::update and
camera basis, among them an axis-aligned camera (exact-zero direction components: the NaN rule of DESIGN.md §3).
"""
import copy

import numpy as np
import pytest

import util
from test_gpu_parity import MODES          # every launch shape rtx_render_tiles knows

pytestmark = pytest.mark.gpu

FOV = float(np.float32(110.0) * np.float32(3.14159265359) * np.float32(0.00555555555))      # Camera.h default, as test_host uses it
SCENE_VIEW = 2                                                                               # index of the scene's own camera in camera_set


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def camera_set(sc):
    """(V,) scene_io.CAMERA: moved / rotated cameras around the scene's own one, which is view SCENE_VIEW."""
    from pyrtx import host
    from pyrtx import scene_io as sio
    W, H = sc.width, sc.height
    pos = sc.camera["position"][0].astype(np.float32)
    cams = []
    moved = sc.camera.copy(); moved["position"] = pos + np.float32([0.25, 0.1, -0.2])        # the scene's view, moved
    cams.append(moved[0])
    p, r = host.camera_update(0.05, ["W", "LEFT"], pos, host.axis_angle((0, 1, 0), 0.35))
    cams.append(host.camera_basis(W, H, FOV, p, r)[0])
    cams.append(sc.camera[0])
    cams.append(host.camera_basis(W, H, FOV, pos, (0, 0, 0, 1))[0])                         # axis-aligned
    p, r = host.camera_update(0.1, ["S", "UP", "LSHIFT"], pos, host.axis_angle((1, 0, 0), -0.25))
    cams.append(host.camera_basis(W, H, FOV, p, r)[0])
    p, r = host.camera_update(0.05, ["D", "DOWN"], pos, host.axis_angle((0, 1, 0), 2.5))    # turned round
    cams.append(host.camera_basis(W, H, FOV, p, r)[0])
    out = np.array(cams, dtype=sio.CAMERA)
    assert out[SCENE_VIEW].tobytes() == sc.camera[0].tobytes()
    return out


def with_camera(sc, cam):
    s = copy.copy(sc)
    s.camera = np.array([cam], dtype=sc.camera.dtype)
    return s


def single_views(api, sc, cams, **flags):
    """One rtx_set_frame + rtx_render_tiles render per camera, on one context."""
    r = api.Renderer(sc)
    outs = []
    for k in range(len(cams)):
        r.set_frame(with_camera(sc, cams[k]))
        outs.append(r.render(**flags))
    r.close()
    return outs


def assert_views_equal(views, singles, first_view=0, work=False):
    for k, s in enumerate(singles):
        v = first_view + k
        assert util.bit_exact(views["rgb"][k], s["rgb"]), f"view {v}: rgb differs from its single-view render"
        assert np.array_equal(views["packed"][k], s["packed"]), f"view {v}: packed differs from its single-view render"
    for key in ("primary", "shadow", "reflection", "refraction"):
        assert views["stats"][key] == sum(s["stats"][key] for s in singles), (key, views["stats"], [s["stats"] for s in singles])
    if work:
        for key in singles[0]["work"]:
            assert views["work"][key] == sum(s["work"][key] for s in singles), key


def render_all_views(api, sc, cams, **flags):
    r = api.Renderer(sc)
    r.set_views(cams)
    out = r.render_views(**flags)
    r.close()
    return out


@pytest.mark.parametrize("name", ["cube", "monkey_small", "materials_aniso", "materials_ewa", "dynamic", "tori16"])
def test_views_bit_exact_vs_single_view_and_oracle(api, name):
    import orc
    sc, g = util.load_golden(name)
    cams = camera_set(sc)
    out = render_all_views(api, sc, cams)
    assert out["rgb"].shape == (len(cams), sc.height, sc.width, 3) and out["packed"].shape == (len(cams), sc.height, sc.width)
    singles = single_views(api, sc, cams)
    assert_views_equal(out, singles)
    for k in range(len(cams)):
        ref = orc.OracleScene(with_camera(sc, cams[k])).render(threads=8)
        assert util.bit_exact(out["rgb"][k], ref["rgb"]), f"view {k}: rgb differs from the oracle"
        assert np.array_equal(out["packed"][k], ref["packed"]), f"view {k}: packed differs from the oracle"
        assert singles[k]["stats"] == ref["stats"], k
    cmp = util.compare_to_golden({"rgb": out["rgb"][SCENE_VIEW], "packed": out["packed"][SCENE_VIEW], "stats": singles[SCENE_VIEW]["stats"]}, g)
    assert cmp["bit_exact"] and cmp["packed_mismatch"] == 0 and cmp["stats_equal"], cmp
    # the views differ from each other: the comparison above is not comparing one image six times
    assert len({out["packed"][k].tobytes() for k in range(len(cams))}) == len(cams)


LAUNCH_SHAPES = dict(MODES, count_work={"count_work": True}, packet_stats={"packet_stats": True})


@pytest.mark.parametrize("mode", list(LAUNCH_SHAPES))
@pytest.mark.parametrize("name", ["materials_aniso", "dynamic"])
def test_views_every_launch_shape(api, name, mode):
    flags = LAUNCH_SHAPES[mode]
    sc, _ = util.load_golden(name)
    cams = camera_set(sc)
    out = render_all_views(api, sc, cams, **flags)
    assert_views_equal(out, single_views(api, sc, cams, **flags), work=mode == "count_work")


@pytest.mark.parametrize("name", ["monkey_small_heat", "materials_heat", "materials_b5"])
def test_views_heatmap_and_deep_configs(api, name):
    sc, g = util.load_golden(name)
    cams = camera_set(sc)
    out = render_all_views(api, sc, cams)
    singles = single_views(api, sc, cams)
    assert_views_equal(out, singles)
    cmp = util.compare_to_golden({"rgb": out["rgb"][SCENE_VIEW], "packed": out["packed"][SCENE_VIEW], "stats": singles[SCENE_VIEW]["stats"]}, g)
    assert cmp["bit_exact"] and cmp["packed_mismatch"] == 0 and cmp["stats_equal"], cmp


@pytest.mark.parametrize("name", ["materials_aniso", "dynamic"])
def test_views_batches_straddle_views_at_an_odd_resolution(api, name, monkeypatch):
    """100x70: 4 x 3 tiles per view, the right and bottom ones clipped; 5 tiles per batch at 3 bounces, so batches straddle views."""
    monkeypatch.setenv("RTX_SLOT_BUDGET", str(1024 * 15 * 5))
    sc, _ = util.load_golden(name)
    sc.config["width"] = 100; sc.config["height"] = 70
    assert sc.tile_count == 12 and int(sc.config["bounces"][0]) == 3
    cams = camera_set(sc)
    for flags in ({}, {"serial": True}, {"lane_trace": True}):
        out = render_all_views(api, sc, cams, **flags)
        assert_views_equal(out, single_views(api, sc, cams, **flags))
    r = api.Renderer(sc)                        # a sub-range starting inside the set
    r.set_views(cams)
    part = r.render_views(3, 2)
    assert_views_equal(part, single_views(api, sc, cams[3:5]), first_view=3)


def test_views_isolation_and_ordering(api):
    import torch
    sc, _ = util.load_golden("materials_aniso")
    cams = camera_set(sc)
    other = cams[::-1].copy()
    singles = single_views(api, sc, cams)
    singles_other = single_views(api, sc, other)
    r = api.Renderer(sc)
    before = r.render()
    r.set_views(cams)
    full = r.render_views()
    assert_views_equal(full, singles)
    # views 2 and 3 with other cameras: the other views' pixels and the single framebuffer are untouched
    r.set_views(other)
    part = r.render_views(2, 2)
    assert_views_equal(part, singles_other[2:4], first_view=2)
    rgb, packed = r.read_views(0, len(cams))
    for k in range(len(cams)):
        want = singles_other[k] if k in (2, 3) else singles[k]
        assert util.bit_exact(rgb[k], want["rgb"]) and np.array_equal(packed[k], want["packed"]), k
    fb_rgb, fb_packed = r.framebuffer()
    assert util.bit_exact(fb_rgb, before["rgb"]) and np.array_equal(fb_packed, before["packed"])
    # rtx_render_tiles afterwards: the rtx_set_frame camera's image, whatever views are set
    after = r.render()
    assert util.bit_exact(after["rgb"], before["rgb"]) and np.array_equal(after["packed"], before["packed"]) and after["stats"] == before["stats"]
    # set_views(A); render; set_views(B); render with no synchronisation in between
    V, H, W = len(cams), sc.height, sc.width
    ta = (torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((V, H, W), dtype=torch.int32, device="cuda"))
    tb = (torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((V, H, W), dtype=torch.int32, device="cuda"))
    r.set_views(cams)
    r.render_views_into(*ta)
    r.set_views(other)
    r.render_views_into(*tb)
    torch.cuda.synchronize()
    for k in range(V):
        assert util.bit_exact(ta[0][k].cpu().numpy(), singles[k]["rgb"]) and np.array_equal(ta[1][k].cpu().numpy().view(np.uint32), singles[k]["packed"]), k
        assert util.bit_exact(tb[0][k].cpu().numpy(), singles_other[k]["rgb"]) and np.array_equal(tb[1][k].cpu().numpy().view(np.uint32), singles_other[k]["packed"]), k
    r.close()


@pytest.mark.parametrize("name", ["materials_aniso", "tori16"])
def test_views_graph_replay_with_changing_cameras(api, name, monkeypatch):
    """RTX_GRAPH=1: identical calls replay a captured hipGraph; the cameras are read from device memory at replay."""
    monkeypatch.setenv("RTX_GRAPH", "1")
    sc, _ = util.load_golden(name)
    cams = camera_set(sc)
    singles = single_views(api, sc, cams)
    r = api.Renderer(sc)
    n = 4
    for it in range(6):
        order = [(it + k) % len(cams) for k in range(n)]
        r.set_views(cams[order])
        out = r.render_views()
        assert_views_equal(out, [singles[k] for k in order])
    r.set_views(cams[:n])                      # a different view range is a different call
    out = r.render_views(1, 2)
    assert_views_equal(out, singles[1:3], first_view=1)
    single = r.render()                        # and a tiles call is not a view call
    assert np.array_equal(single["packed"], singles[SCENE_VIEW]["packed"])
    r.close()


def test_render_views_into_torch_tensors(api):
    import torch
    sc, _ = util.load_golden("dynamic")
    cams = camera_set(sc)
    r = api.Renderer(sc)
    r.set_views(cams)
    ref = r.render_views()
    V, H, W = len(cams), sc.height, sc.width
    rgb = torch.full((V + 2, H, W, 3), -1.0, dtype=torch.float32, device="cuda")       # capacity larger than the views rendered
    packed = torch.full((V + 2, H, W), -1, dtype=torch.int32, device="cuda")
    r.render_views_into(rgb, packed)
    torch.cuda.synchronize()
    assert util.bit_exact(rgb[:V].cpu().numpy(), ref["rgb"])
    assert np.array_equal(packed[:V].cpu().numpy().view(np.uint32), ref["packed"])
    assert bool((rgb[V:] == -1.0).all()) and bool((packed[V:] == -1).all())
    assert r.stats()[0] == ref["stats"]
    # a sub-range into a second pair of tensors, then back to the context's own buffers
    rgb2 = torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"); packed2 = torch.zeros((V, H, W), dtype=torch.int32, device="cuda")
    r.render_views_into(rgb2, packed2, first_view=1, view_count=3)
    torch.cuda.synchronize()
    assert util.bit_exact(rgb2[1:4].cpu().numpy(), ref["rgb"][1:4]) and bool((rgb2[0] == 0).all()) and bool((rgb2[4:] == 0).all())
    again = r.render_views()
    assert util.bit_exact(again["rgb"], ref["rgb"]) and np.array_equal(again["packed"], ref["packed"])
    r.close()


def test_render_views_into_is_ordered_on_torch_streams(api):
    """No device-wide synchronisation: torch work queued before render_views_into on the current stream (tens of milliseconds of matrix
    products, then a fill of the tensors) must land before the render, torch work queued after it (a copy of the tensors) must see the
    finished images — on torch's default stream (handle 0) and on a stream of its own.  Unordered, the late fill would overwrite the
    images, or the copy would take the fill or a partial image."""
    import torch
    from pyrtx import host
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    cams = camera_set(sc)[1:5]
    r = api.Renderer(sc)
    r.set_views(cams)
    ref = r.render_views()
    V, H, W = len(cams), sc.height, sc.width
    a = torch.randn(4096, 4096, device="cuda"); b = torch.randn(4096, 4096, device="cuda"); c = torch.empty_like(a)
    torch.cuda.synchronize()
    for own_stream in (False, True):
        s = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
        assert own_stream or s.cuda_stream == 0
        with torch.cuda.stream(s):
            rgb = torch.empty((V, H, W, 3), dtype=torch.float32, device="cuda"); packed = torch.empty((V, H, W), dtype=torch.int32, device="cuda")
            for _ in range(40):
                torch.mm(a, b, out=c)                             # keeps the stream busy
            rgb.fill_(-1.0); packed.fill_(-1)                     # queued before the render
            r.render_views_into(rgb, packed)
            snap_rgb, snap_packed = rgb.clone(), packed.clone()   # queued after the render
            for _ in range(40):
                torch.mm(a, b, out=c)
            got_rgb, got_packed = snap_rgb.cpu().numpy(), snap_packed.cpu().numpy()
            now_rgb = rgb.cpu().numpy()
        assert util.bit_exact(got_rgb, ref["rgb"]), f"own_stream={own_stream}: the copy queued after the render did not see the images"
        assert np.array_equal(got_packed.view(np.uint32), ref["packed"]), own_stream
        assert util.bit_exact(now_rgb, ref["rgb"]), f"own_stream={own_stream}: the fill queued before the render landed after it"
    r.close()


def test_views_full_size_atrium(api):
    """cfg3 atrium at 1080p, 3 views in one call: the packet kernels at full size."""
    from pyrtx import host
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    cams = camera_set(sc)[1:4]
    out = render_all_views(api, sc, cams)
    assert_views_equal(out, single_views(api, sc, cams))


def test_views_error_codes(api):
    import torch
    from pyrtx import scene_io as sio
    INVALID, STATE = 1, 5
    sc, _ = util.load_golden("cube")
    cams = camera_set(sc)[:3]
    singles = single_views(api, sc, cams)
    lib = api.load_library()

    r0 = api.Renderer(sc, upload=False)          # no rtx_set_frame yet
    assert lib.rtx_set_views(r0.ctx, cams.ctypes.data, 3) == 0
    assert lib.rtx_render_views(r0.ctx, 0, 3, 0) == STATE
    r0.close()

    r = api.Renderer(sc)
    assert lib.rtx_render_views(r.ctx, 0, 1, 0) == STATE                 # before rtx_set_views
    assert lib.rtx_set_views(r.ctx, cams.ctypes.data, 0) == INVALID
    assert lib.rtx_set_views(r.ctx, None, 3) == INVALID
    many = np.repeat(cams[:1], api.RTX_MAX_VIEWS + 1)
    assert lib.rtx_set_views(r.ctx, many.ctypes.data, api.RTX_MAX_VIEWS + 1) == INVALID
    assert lib.rtx_set_views(r.ctx, cams.ctypes.data, 3) == 0
    assert lib.rtx_render_views(r.ctx, 0, 0, 0) == INVALID
    assert lib.rtx_render_views(r.ctx, -1, 2, 0) == INVALID
    assert lib.rtx_render_views(r.ctx, 2, 2, 0) == INVALID               # outside the views set
    assert lib.rtx_render_views(r.ctx, 0, api.RTX_MAX_VIEWS + 1, 0) == INVALID
    assert lib.rtx_read_views(r.ctx, 1, 3, None, None) == INVALID
    assert lib.rtx_read_views(r.ctx, 0, 0, None, None) == INVALID
    H, W = sc.height, sc.width
    small = (torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((2, H, W), dtype=torch.int32, device="cuda"))
    assert lib.rtx_bind_view_framebuffer(r.ctx, small[0].data_ptr(), None, 2) == INVALID
    assert lib.rtx_bind_view_framebuffer(r.ctx, small[0].data_ptr(), small[1].data_ptr(), 0) == INVALID
    assert lib.rtx_bind_view_framebuffer(r.ctx, small[0].data_ptr(), small[1].data_ptr(), 2) == 0
    assert lib.rtx_render_views(r.ctx, 0, 3, 0) == INVALID               # bound capacity too small
    assert lib.rtx_read_views(r.ctx, 0, 3, None, None) == INVALID
    assert lib.rtx_bind_view_framebuffer(r.ctx, None, None, 0) == 0
    # the context still renders correctly
    r.bind_view_framebuffer(None, None)
    r.set_views(cams)
    out = r.render_views()
    assert_views_equal(out, singles)
    r.close()

    # view_count * width * height >= 2^31: 1036 views of 1920x1080
    big = copy.copy(sc); big.config = sc.config.copy(); big.config["width"] = 1920; big.config["height"] = 1080
    rb = api.Renderer(big)
    n = (1 << 31) // (1920 * 1080) + 1
    cam_n = np.repeat(cams[:1], n).astype(sio.CAMERA)
    assert lib.rtx_set_views(rb.ctx, cam_n.ctypes.data, n) == INVALID
    assert lib.rtx_set_views(rb.ctx, cam_n.ctypes.data, n - 1) == 0
    assert lib.rtx_render_views(rb.ctx, 0, n, 0) == INVALID
    rb.close()
