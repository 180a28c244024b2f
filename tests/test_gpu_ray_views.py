"""Ray views: caller-supplied primary rays (include/rtx.h rtx_set_rays / rtx_bind_rays / rtx_render_rays).

Everything is compared bit for bit (float arrays as uint32, NaN == NaN), with no tolerance and no excluded sample:
  * the rays of a pinhole camera (pyrtx.api.pinhole_rays) render the camera's own frame: colour, packed pixels, ray counts, AOVs and work
    counters, in every launch shape;
  * V ray views of V cameras equal rtx_render_views of those cameras;
  * a seeded permutation of all rays of several cameras renders the permuted pixels: every pixel depends on its own ray only (the yardstick
    for ray sets that are no camera's), which also drives fully incoherent level-0 packets through every kernel family;
  * rays with a zero direction are no rays: their pixels are left alone and they are not counted;
  * adversarial rays (tests/rayset.py, plus NaN / inf rays) and an orthographic grid: the primary-hit AOVs equal rtx_debug_trace_rays
    and the oracle;
  * state, errors, rebinding with work queued, hipGraph replay and several contexts in flight.
The COLOUR of rays that are no camera's (origins of their own, so the per-ray camera at depth >= 1; adversarial materials and lights) is
compared with the oracle and the reference's records in tests/test_gpu_shade_rays.py.
"""
import ctypes as C

import numpy as np
import pytest

import util
from test_gpu_parity import MODES          # every launch shape rtx_render_tiles knows
from test_gpu_views import camera_set

pytestmark = pytest.mark.gpu

f32 = np.float32
ALL = ("depth", "position", "normal", "albedo", "uv", "material_id", "object_id", "triangle_id")
STATS = ("primary", "shadow", "reflection", "refraction")
INVALID, STATE = 1, 5


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def load(name):
    if name == "ragged":                       # 100x70: edge tiles clipped in both directions
        sc, _ = util.load_golden("materials_aniso")
        sc.config["width"] = 100; sc.config["height"] = 70
        return sc
    return util.load_golden(name)[0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def assert_same(a, b, what=""):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = bits(a) != bits(b)
    if a.dtype == np.float32:
        bad &= ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


def camera_rays(api, sc, cams):
    return np.stack([api.pinhole_rays(c, sc.width, sc.height) for c in cams])


def assert_frame(out, ref, k=0, what="", aovs=ALL):
    """ray view k of `out` against the tiles-call frame `ref`"""
    assert_same(out["rgb"][k], ref["rgb"], what + " rgb")
    assert_same(out["packed"][k], ref["packed"], what + " packed")
    for ch in aovs:
        assert_same(out[ch][k], ref[ch], f"{what} {ch}")


# ---- 4: pinhole identity ----------------------------------------------------------------------------------------------------------------
PINHOLE_SCENES = [n for n in util.GOLDENS if not n.endswith("_heat")] + ["ragged"]
SHAPES = dict(MODES, count_work={"count_work": True}, simple={"simple_trace": True}, packet_stats={"packet_stats": True})
KNOBS = {"fuse": {"RTX_FUSE_SHADE": "1"}, "lpt0": {"RTX_PK_LPT": "0"}, "lpt1": {"RTX_PK_LPT": "1"}}


def pinhole_identity(api, sc, flags, repeats=1):
    r = api.Renderer(sc)
    rays = api.pinhole_rays(sc.camera[0], sc.width, sc.height)
    r.set_rays(rays)
    for it in range(repeats):              # RTX_PK_LPT orders a call by the cost of the previous call of its own key space
        ref = r.render(**flags)
        out = r.render_rays(**flags)
        assert out["rgb"].shape == (1, sc.height, sc.width, 3)
        assert_frame(out, ref, 0, f"call {it}", aovs=())
        assert out["stats"] == ref["stats"], (out["stats"], ref["stats"])
        assert out["stats"]["primary"] == sc.width * sc.height
        if flags.get("count_work"):
            assert out["work"] == ref["work"], {k: (out["work"][k], ref["work"][k]) for k in ref["work"] if out["work"][k] != ref["work"][k]}
        ref_a = r.render_aovs(ALL, **flags)
        out_a = r.render_rays(aovs=ALL, **flags)
        assert_frame(out_a, ref_a, 0, f"call {it} (AOV)")
        assert_same(out_a["rgb"], out["rgb"], "AOV call rgb")
        assert out_a["stats"] == ref["stats"]
    r.close()


@pytest.mark.parametrize("mode", list(SHAPES))
@pytest.mark.parametrize("name", PINHOLE_SCENES)
def test_pinhole_rays_render_the_cameras_frame(api, name, mode):
    pinhole_identity(api, load(name), SHAPES[mode])


@pytest.mark.parametrize("mode", ["default", "serial", "serial_cull"])
@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("name", PINHOLE_SCENES)
def test_pinhole_rays_with_fused_shading_and_longest_first(api, name, knob, mode, monkeypatch):
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    pinhole_identity(api, load(name), MODES[mode], repeats=3 if knob.startswith("lpt") else 1)


# ---- 5: ray views = camera views ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["materials_aniso", "tori16", "ragged"])
def test_ray_views_equal_camera_views(api, name):
    import torch
    sc = load(name)
    cams = camera_set(sc)[:5]
    V, H, W = len(cams), sc.height, sc.width
    r = api.Renderer(sc)
    r.set_views(cams)
    ref = r.render_views(aovs=ALL)
    rays = camera_rays(api, sc, cams)
    r.set_rays(rays)
    out = r.render_rays(aovs=ALL)
    for ch in ("rgb", "packed") + ALL:
        assert_same(out[ch], ref[ch], ch)
    assert out["stats"] == ref["stats"]
    assert len({out["packed"][k].tobytes() for k in range(V)}) >= V - 1          # the views differ: not one image compared five times
    # a sub-range: ray view v is pixel range [v * W * H, (v + 1) * W * H) of the view framebuffer and of the AOVs
    part_ref = r.render_views(1, 3, aovs=("depth", "object_id"), serial=True)
    part = r.render_rays(1, 3, aovs=("depth", "object_id"), serial=True)
    for ch in ("rgb", "packed", "depth", "object_id"):
        assert_same(part[ch], ref[ch][1:4], "sub-range " + ch)
    assert part["stats"] == part_ref["stats"]
    # caller tensors of larger capacity: the pixels outside the rendered range stay as they are
    from pyrtx.ctypes_structs import AOV_CHANNELS
    cap = V + 2
    rgb = torch.full((cap, H, W, 3), -1.0, dtype=torch.float32, device="cuda"); packed = torch.full((cap, H, W), -1, dtype=torch.int32, device="cuda")
    aovs = {ch: torch.full(api.aov_shape(ch, cap, H, W), -3, dtype=torch.float32 if AOV_CHANNELS[ch][1] == np.float32 else torch.int32, device="cuda") for ch in ALL}
    dev_rays = torch.from_numpy(rays[:3]).cuda()
    r.render_rays_into(rgb, packed, dev_rays, aovs=aovs)
    torch.cuda.synchronize()
    assert_same(rgb[:3].cpu().numpy(), ref["rgb"][:3], "into rgb"); assert_same(packed[:3].cpu().numpy().view(np.uint32), ref["packed"][:3], "into packed")
    assert bool((rgb[3:] == -1.0).all()) and bool((packed[3:] == -1).all())
    for ch in ALL:
        assert_same(aovs[ch][:3].cpu().numpy(), ref[ch][:3], "into " + ch)
        assert bool((aovs[ch][3:] == -3).all()), ch
    # a range inside bound rays and tensors through the C ABI: views 1..2 of five bound ray views
    rgb.fill_(-1.0); packed.fill_(-1); torch.cuda.synchronize()
    dev_all = torch.from_numpy(rays).cuda()
    r.bind_aovs(0)
    r.bind_rays(dev_all, V)
    r.render_rays_async(1, 2)
    r.synchronize()
    assert_same(rgb[1:3].cpu().numpy(), ref["rgb"][1:3], "bound sub-range")
    assert bool((rgb[0] == -1.0).all()) and bool((rgb[3:] == -1.0).all()) and bool((packed[0] == -1).all()) and bool((packed[3:] == -1).all())
    r.close()


# ---- 6: every pixel depends on its own ray only ---------------------------------------------------------------------------------------
PERM_MODES = {"default": {}, "serial": {"serial": True}, "lane": {"lane_trace": True}, "simple": {"simple_trace": True}}
_PERM = {}


def permuted_set(api, name):
    """(scene, cameras, render_views result with every AOV, rays (V, H, W, 18) permuted over the whole set, permutation)"""
    if name not in _PERM:
        sc = load(name)
        cams = camera_set(sc)[[0, 2, 5]]          # the scene's view moved, the scene's own view, one turned round
        r = api.Renderer(sc)
        r.set_views(cams)
        ref = r.render_views(aovs=ALL)
        r.close()
        rays = camera_rays(api, sc, cams)
        perm = np.random.default_rng(2024).permutation(rays.shape[0] * sc.height * sc.width)
        _PERM[name] = (sc, cams, ref, np.ascontiguousarray(rays.reshape(-1, 18)[perm].reshape(rays.shape)), perm)
    return _PERM[name]


@pytest.mark.parametrize("mode", list(PERM_MODES))
@pytest.mark.parametrize("name", ["materials_aniso", "tori16"])
def test_permuted_rays_render_the_permuted_pixels(api, name, mode):
    sc, cams, ref, rays, perm = permuted_set(api, name)
    assert len({ref["packed"][k].tobytes() for k in range(len(cams))}) == len(cams)
    r = api.Renderer(sc)
    r.set_rays(rays)
    out = r.render_rays(aovs=ALL, **PERM_MODES[mode])
    r.close()
    n = perm.size
    for ch in ("rgb", "packed") + ALL:
        got = out[ch].reshape(n, -1); want = ref[ch].reshape(n, -1)[perm]
        assert_same(got, want, ch)
    assert out["stats"] == ref["stats"], (out["stats"], ref["stats"])


# ---- 7: inactive rays ---------------------------------------------------------------------------------------------------------------------
def inactive_mask(V, H, W, seed):
    """~30 % of the pixels: single pixels, whole 8x8 blocks and whole 32x32 tiles"""
    rng = np.random.default_rng(seed)
    m = rng.random((V, H, W)) < 0.12
    for v in range(V):
        for _ in range(max(2, (H // 8) * (W // 8) // 8)):
            y, x = int(rng.integers(0, (H + 7) // 8)) * 8, int(rng.integers(0, (W + 7) // 8)) * 8
            m[v, y:y + 8, x:x + 8] = True
        for _ in range(max(1, ((H + 31) // 32) * ((W + 31) // 32) // 10)):
            y, x = int(rng.integers(0, (H + 31) // 32)) * 32, int(rng.integers(0, (W + 31) // 32)) * 32
            m[v, y:y + 32, x:x + 32] = True
    return m


@pytest.mark.parametrize("flags", [{}, {"serial": True, "lane_trace": True}, {"simple_trace": True}], ids=["default", "serial_lane", "simple"])
@pytest.mark.parametrize("name", ["materials_aniso", "ragged"])
def test_inactive_rays_write_nothing_and_are_not_counted(api, name, flags):
    import torch
    from pyrtx.ctypes_structs import AOV_CHANNELS
    sc = load(name)
    cams = camera_set(sc)[1:3]
    V, H, W = len(cams), sc.height, sc.width
    rays = camera_rays(api, sc, cams)
    mask = inactive_mask(V, H, W, 11)
    frac = mask.mean()
    assert 0.2 < frac < 0.45, frac
    masked = rays.copy()
    zeros = np.random.default_rng(3).choice(np.array([0.0, -0.0], f32), size=(int(mask.sum()), 3))
    masked[mask, 3:6] = zeros
    assert np.signbit(masked[mask, 3:6]).any() and not masked[mask, 3:6].any()

    def tensors():
        rgb = torch.full((V, H, W, 3), -5.5, dtype=torch.float32, device="cuda"); packed = torch.full((V, H, W), -9, dtype=torch.int32, device="cuda")
        aovs = {ch: torch.full(api.aov_shape(ch, V, H, W), -3, dtype=torch.float32 if AOV_CHANNELS[ch][1] == np.float32 else torch.int32, device="cuda") for ch in ALL}
        return rgb, packed, aovs

    r = api.Renderer(sc)
    full = tensors(); part = tensors()
    r.render_rays_into(full[0], full[1], torch.from_numpy(rays).cuda(), aovs=full[2], **flags)
    torch.cuda.synchronize()
    full_stats = r.stats()[0]
    r.render_rays_into(part[0], part[1], torch.from_numpy(masked).cuda(), aovs=part[2], **flags)
    torch.cuda.synchronize()
    stats = r.stats()[0]
    assert full_stats["primary"] == V * H * W
    assert stats["primary"] == int((~mask).sum()), (stats, int((~mask).sum()))
    assert stats["shadow"] <= full_stats["shadow"]
    for what, a, b, fill in [("rgb", part[0], full[0], -5.5), ("packed", part[1], full[1], -9)] + [(ch, part[2][ch], full[2][ch], -3) for ch in ALL]:
        a = a.cpu().numpy(); b = b.cpu().numpy()
        assert_same(a[~mask], b[~mask], what + " of the live rays")
        assert (bits(a[mask]) == bits(np.full_like(a[mask], fill))).all(), f"{what}: a pixel without a ray was written"
    r.close()


# ---- 8: arbitrary rays, first hit --------------------------------------------------------------------------------------------------------
def adversarial_rays(sc, o, W, H):
    """(H * W, 18) rays: the classes of tests/rayset.py and a class with NaN / inf origin and direction components, padded with inactive
    rays and shuffled by a seeded permutation; and the live mask."""
    import rayset
    rays = rayset.generate(sc, 192, 21, o)[0]
    rng = np.random.default_rng(77)
    odd = rays[rng.integers(len(rays), size=160)].copy()
    special = np.array([np.nan, np.inf, -np.inf], f32)
    for i in range(len(odd)):
        cols = rng.choice(6, size=int(rng.integers(1, 3)), replace=False)
        odd[i, cols] = special[rng.integers(3, size=len(cols))]
    rays = np.concatenate([rays, odd]).astype(f32)
    assert len(rays) <= W * H
    out = np.zeros((W * H, 18), f32)
    out[:len(rays)] = rays
    live = np.zeros(W * H, bool); live[:len(rays)] = True
    live &= (out[:, 3:6] != 0).any(axis=1) | np.isnan(out[:, 3:6]).any(axis=1)      # a generated ray with a zero direction is inactive too
    p = rng.permutation(W * H)
    return np.ascontiguousarray(out[p]), live[p]


def orthographic_rays(api, sc):
    """every ray has its own origin: a grid in the plane through the camera, along the camera's central direction"""
    H, W = sc.height, sc.width
    pin = api.pinhole_rays(sc.camera[0], W, H)
    centre = pin[H // 2, W // 2, 3:6]
    cam = sc.camera[0]
    ax, ay = np.asarray(cam["rotated_x_axis"], f32), np.asarray(cam["rotated_y_axis"], f32)
    j, i = np.meshgrid(np.arange(H, dtype=f32) - f32(H / 2), np.arange(W, dtype=f32) - f32(W / 2), indexing="ij")
    scale = f32(6.0 / W) / np.sqrt((ax * ax).sum())
    o = np.asarray(cam["position"], f32) + (ax * i[..., None] + ay * j[..., None]) * scale
    return api.rays_from_directions(o.astype(f32), np.broadcast_to(centre, o.shape)).reshape(-1, 18), np.ones(H * W, bool)


@pytest.mark.parametrize("kind", ["adversarial", "orthographic"])
@pytest.mark.parametrize("name", ["materials_aniso", "tori16", "coincident"])
def test_arbitrary_rays_first_hit_equals_debug_trace_and_oracle(api, name, kind):
    """Rays that are no camera's, as level-0 rays: the primary-hit AOVs against the oracle's trace_closest (every live ray) and against
    rtx_debug_trace_rays (every live ray with finite origin and direction: that hook queues its rays at level 1, where the packet kernel's
    walk of a NaN origin does not end — see ray_is_finite, csrc/rtx_trace.h; a ray call does not walk such rays, and they hit nothing)."""
    import orc
    from test_gpu_rays import traceable
    sc = traceable(load(name))
    H, W = sc.height, sc.width
    o = orc.OracleScene(sc)
    rays, live = adversarial_rays(sc, o, W, H) if kind == "adversarial" else orthographic_rays(api, sc)
    assert live.sum() > 1000
    finite = np.isfinite(rays[:, :6]).all(axis=1)
    if kind == "adversarial":
        assert (live & ~finite).sum() > 100 and (~live).sum() > 1000
    want, _ = o.trace_closest(rays[live], 8)
    assert not (want[~finite[live], 0] > 0).any(), "a ray with a non-finite component hits nothing in the reference's arithmetic"
    r = api.Renderer(sc)
    r.set_rays(rays.reshape(H, W, 18))
    outs = {m: r.render_rays(aovs=ALL, **fl) for m, fl in (("default", {}), ("simple", {"simple_trace": True}), ("lane", {"lane_trace": True}))}
    dbg = r.debug_trace_rays(rays[live & finite])
    r.close()
    util.check_hits(dbg, want[finite[live]])
    for m, out in outs.items():
        assert out["stats"]["primary"] == int(live.sum()), m
        for ch in ("rgb", "packed") + ALL:
            assert_same(out[ch], outs["default"][ch], f"{m} vs default: {ch}")
    out = outs["default"]
    for ref, sel, what in ((dbg, live & finite, "rtx_debug_trace_rays"), (want, live, "oracle")):
        flat = lambda ch: out[ch].reshape(H * W, -1)[sel]
        hit = ref[:, 0] > 0
        assert hit.any() and ((~hit).any() or kind == "orthographic"), "the adversarial sets hold hits and misses (depth inf, material_id -1)"
        assert_same(flat("depth")[:, 0], np.where(hit, ref[:, 1], f32(np.inf)).astype(f32), f"depth vs {what}")
        assert_same(flat("position")[hit], ref[hit, 2:5], f"position vs {what}")
        assert_same(flat("normal")[hit], ref[hit, 5:8], f"normal vs {what}")
        assert_same(flat("uv")[hit], ref[hit, 9:11], f"uv vs {what}")
        assert_same(flat("material_id").view(np.int32)[hit, 0], ref[hit, 8].astype(np.int32), f"material_id vs {what}")
        assert (flat("material_id").view(np.int32)[~hit] == -1).all()


# ---- 9: state and errors ------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_state(api):
    import copy
    import torch
    sc = load("cube")
    H, W = sc.height, sc.width
    lib = api.load_library()
    cams = camera_set(sc)[:3]
    rays = camera_rays(api, sc, cams)
    dev = torch.from_numpy(rays).cuda()

    r0 = api.Renderer(sc, upload=False)                                   # no rtx_set_frame yet
    assert lib.rtx_set_rays(r0.ctx, rays.ctypes.data, 3) == 0
    assert lib.rtx_render_rays(r0.ctx, 0, 3, 0) == STATE
    r0.close()

    r = api.Renderer(sc)
    before = r.render()
    assert lib.rtx_render_rays(r.ctx, 0, 1, 0) == STATE                   # before any rays are set or bound
    assert lib.rtx_set_rays(r.ctx, rays.ctypes.data, 0) == INVALID
    assert lib.rtx_set_rays(r.ctx, None, 3) == INVALID
    assert lib.rtx_set_rays(r.ctx, rays.ctypes.data, api.RTX_MAX_VIEWS + 1) == INVALID
    assert lib.rtx_bind_rays(r.ctx, dev.data_ptr(), 0) == INVALID
    assert lib.rtx_bind_rays(r.ctx, dev.data_ptr(), api.RTX_MAX_VIEWS + 1) == INVALID
    assert lib.rtx_bind_rays(r.ctx, dev.data_ptr() + 4, 1) == INVALID     # not 8-byte aligned
    assert lib.rtx_render_rays(r.ctx, 0, 1, 0) == STATE
    assert lib.rtx_set_rays(r.ctx, rays.ctypes.data, 3) == 0
    assert lib.rtx_render_rays(r.ctx, 0, 0, 0) == INVALID
    assert lib.rtx_render_rays(r.ctx, -1, 2, 0) == INVALID
    assert lib.rtx_render_rays(r.ctx, 2, 2, 0) == INVALID                 # outside the rays set
    assert lib.rtx_render_rays(r.ctx, 0, api.RTX_MAX_VIEWS + 1, 0) == INVALID
    assert lib.rtx_bind_rays(r.ctx, dev.data_ptr(), 2) == 0               # bound rays take the place of the set ones: two views
    assert lib.rtx_render_rays(r.ctx, 0, 3, 0) == INVALID
    assert lib.rtx_render_rays(r.ctx, 0, 2, 0) == 0
    assert lib.rtx_bind_rays(r.ctx, None, 0) == 0                         # unbound: the three set views are current again
    assert lib.rtx_render_rays(r.ctx, 0, 3, 0) == 0
    small = (torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((2, H, W), dtype=torch.int32, device="cuda"))
    assert lib.rtx_bind_view_framebuffer(r.ctx, small[0].data_ptr(), small[1].data_ptr(), 2) == 0
    assert lib.rtx_render_rays(r.ctx, 0, 3, 0) == INVALID                 # outside the bound view framebuffer
    assert lib.rtx_render_rays(r.ctx, 0, 2, 0) == 0
    assert lib.rtx_bind_view_framebuffer(r.ctx, None, None, 0) == 0
    assert lib.rtx_render_rays(r.ctx, 0, 3, api.RTX_RENDER_AOV) == STATE  # nothing bound
    t = torch.zeros(W * H * 2, dtype=torch.float32, device="cuda")
    from pyrtx.ctypes_structs import RtxAovBuffers
    bufs = RtxAovBuffers(); bufs.depth = t.data_ptr()
    assert lib.rtx_bind_aovs(r.ctx, 1, C.byref(bufs), W * H * 2) == 0
    assert lib.rtx_render_rays(r.ctx, 0, 2, api.RTX_RENDER_AOV) == 0
    assert lib.rtx_render_rays(r.ctx, 0, 3, api.RTX_RENDER_AOV) == INVALID      # 3 * W * H pixels > AOV capacity
    assert lib.rtx_render_rays(r.ctx, 2, 1, api.RTX_RENDER_AOV) == INVALID
    r.bind_aovs(0)
    # ray state and view state are independent; nothing leaks into the calls that follow
    r.set_views(cams[::-1].copy())
    views = r.render_views()
    out = r.render_rays(0, 3)
    for k in range(3):
        assert_same(out["rgb"][k], views["rgb"][2 - k], f"ray view {k}")
    views2 = r.render_views()
    assert_same(views2["rgb"], views["rgb"], "views call after a ray call"); assert views2["stats"] == views["stats"]
    after = r.render()
    assert_same(after["rgb"], before["rgb"], "tiles call after a ray call"); assert_same(after["packed"], before["packed"], "packed"); assert after["stats"] == before["stats"]
    r.group_loopback(2)                                                    # the group path: unaffected by the ray state
    assert_same(r.framebuffer()[1], before["packed"], "group loopback after a ray call")
    r.close()

    heat = util.load_golden("materials_heat")[0]                           # heat-map mode: no ray views
    rh = api.Renderer(heat)
    assert lib.rtx_render_rays(rh.ctx, 0, 1, 0) == STATE and b"heat-map" in lib.rtx_last_error(rh.ctx)      # with or without rays
    rh.set_rays(api.pinhole_rays(heat.camera[0], heat.width, heat.height))
    assert lib.rtx_render_rays(rh.ctx, 0, 1, 0) == STATE
    assert lib.rtx_render_tiles(rh.ctx, 0, 1, heat.tile_count, 0) == 0
    rh.close()

    big = copy.copy(sc); big.config = sc.config.copy(); big.config["width"] = 1920; big.config["height"] = 1080      # V * W * H >= 2^31
    rb = api.Renderer(big)
    n = (1 << 31) // (1920 * 1080) + 1
    assert lib.rtx_bind_rays(rb.ctx, dev.data_ptr(), n) == INVALID
    assert lib.rtx_set_rays(rb.ctx, rays.ctypes.data, n) == INVALID        # refused before anything is read
    assert lib.rtx_bind_rays(rb.ctx, dev.data_ptr(), n - 1) == 0           # only recorded: nothing is read until a render call
    assert lib.rtx_render_rays(rb.ctx, 0, n, 0) == INVALID                 # the call's own V * W * H bound, before the range check
    assert lib.rtx_bind_rays(rb.ctx, None, 0) == 0
    rb.close()


def test_read_views_reaches_ray_views_and_keeps_earlier_views(api):
    """rtx_read_views accepts ranges up to the larger of the views set and the ray views; the growth of the context's own view framebuffer
    to the ray views keeps what the earlier views hold."""
    import torch
    sc = load("cube")
    lib = api.load_library()
    cams = camera_set(sc)[:4]
    r = api.Renderer(sc)
    r.set_views(cams[:2])
    views = r.render_views()
    assert lib.rtx_read_views(r.ctx, 0, 3, None, None) == INVALID and b"rtx_set_rays" in lib.rtx_last_error(r.ctx)
    dev = torch.from_numpy(camera_rays(api, sc, cams)).cuda()
    torch.cuda.synchronize()
    r.bind_rays(dev, 4)
    assert lib.rtx_read_views(r.ctx, 0, 5, None, None) == INVALID
    rgb = np.zeros((4, sc.height, sc.width, 3), f32); packed = np.zeros((4, sc.height, sc.width), np.uint32)
    assert lib.rtx_read_views(r.ctx, 0, 4, rgb.ctypes.data, packed.ctypes.data) == 0      # grows the framebuffer: views 0-1 kept, 2-3 zero
    assert_same(rgb[:2], views["rgb"], "earlier views after the growth"); assert_same(packed[:2], views["packed"], "packed")
    assert not rgb[2:].any() and not packed[2:].any()
    out = r.render_rays(2, 2)
    r.set_views(cams)
    want = r.render_views(2, 2)
    assert_same(out["rgb"], want["rgb"], "ray views 2-3")
    r.close()


def test_rebinding_while_work_is_queued(api):
    """bind(A); render; bind(B); render with no synchronisation in between, and set_rays(A); render; set_rays(B); render: queued work keeps
    the rays it was queued with."""
    import torch
    sc = load("materials_aniso")
    cams = camera_set(sc)
    V, H, W = 3, sc.height, sc.width
    ra, rb = camera_rays(api, sc, cams[:3]), camera_rays(api, sc, cams[3:6])
    r = api.Renderer(sc)
    r.set_views(cams)
    ref = r.render_views()
    da, db = torch.from_numpy(ra).cuda(), torch.from_numpy(rb).cuda()
    mk = lambda: (torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((V, H, W), dtype=torch.int32, device="cuda"))
    ta, tb = mk(), mk()
    torch.cuda.synchronize()
    r.render_rays_into(ta[0], ta[1], da)
    r.render_rays_into(tb[0], tb[1], db)
    torch.cuda.synchronize()
    assert_same(ta[0].cpu().numpy(), ref["rgb"][:3], "first binding"); assert_same(tb[0].cpu().numpy(), ref["rgb"][3:6], "second binding")
    assert_same(tb[1].cpu().numpy().view(np.uint32), ref["packed"][3:6], "second binding packed")
    # the own buffer, filled through the staging ring
    r.bind_rays(None)
    tc, td = mk(), mk()
    torch.cuda.synchronize()
    r.bind_view_framebuffer(tc[0].data_ptr(), tc[1].data_ptr(), V)
    r.set_rays(ra); r.render_rays_async()
    r.bind_view_framebuffer(td[0].data_ptr(), td[1].data_ptr(), V)
    r.set_rays(rb); r.render_rays_async()
    r.synchronize(); torch.cuda.synchronize()
    assert_same(tc[0].cpu().numpy(), ref["rgb"][:3], "first set"); assert_same(td[0].cpu().numpy(), ref["rgb"][3:6], "second set")
    r.close()


@pytest.mark.parametrize("name", ["materials_aniso", "tori16"])
def test_graph_replay_rewritten_and_rebound_rays(api, name, monkeypatch):
    """RTX_GRAPH=1: capture, replay, new values in the same buffer, replay, another buffer (never replayed from the first one's graph), each
    equal to an eager render of those rays."""
    import torch
    sc = load(name)
    cams = camera_set(sc)
    sets = [camera_rays(api, sc, cams[[a, b]]) for a, b in ((0, 1), (2, 3), (4, 5), (1, 4))]
    eager = api.Renderer(sc)
    want = []
    for s in sets:
        eager.set_rays(s); want.append(eager.render_rays())
    plain = eager.render()
    eager.close()
    monkeypatch.setenv("RTX_GRAPH", "1")
    r = api.Renderer(sc)
    buf_a = torch.from_numpy(sets[0]).cuda(); buf_b = torch.from_numpy(sets[3]).cuda()
    torch.cuda.synchronize()

    def check(k, what):
        out = r.render_rays()
        assert_same(out["rgb"], want[k]["rgb"], what); assert_same(out["packed"], want[k]["packed"], what); assert out["stats"] == want[k]["stats"], what

    r.bind_rays(buf_a, 2)
    for it in range(3):                                                    # eager, captured, replayed
        check(0, f"buffer a, call {it}")
    for k in (1, 2):                                                       # new values in the same buffer: the replay reads them
        buf_a.copy_(torch.from_numpy(sets[k])); torch.cuda.synchronize()
        check(k, f"buffer a rewritten with set {k}")
    r.bind_rays(buf_b, 2)                                                  # another buffer: a new key
    for it in range(3):
        check(3, f"buffer b, call {it}")
    r.bind_rays(buf_a, 2)
    check(2, "back to buffer a")
    tiles = r.render()                                                     # a tiles call is not a ray call
    assert_same(tiles["rgb"], plain["rgb"], "tiles call"); assert tiles["stats"] == plain["stats"]
    r.bind_rays(None)
    for k in (0, 1, 1, 1, 3):                                              # the own buffer through rtx_set_rays
        r.set_rays(sets[k]); check(k, f"set_rays {k}")
    r.close()


def test_three_contexts_in_flight_on_different_rays(api):
    import torch
    sc = load("materials_aniso")
    cams = camera_set(sc)
    V, H, W = 2, sc.height, sc.width
    ref_r = api.Renderer(sc); ref_r.set_views(cams); ref = ref_r.render_views(); ref_r.close()
    ctxs = [api.Renderer(sc) for _ in range(3)]
    rays = [torch.from_numpy(camera_rays(api, sc, cams[2 * k:2 * k + 2])).cuda() for k in range(3)]
    outs = [(torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"), torch.zeros((V, H, W), dtype=torch.int32, device="cuda")) for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    for rep in range(3):
        for k in range(3):
            with torch.cuda.stream(streams[k]):
                ctxs[k].render_rays_into(outs[k][0], outs[k][1], rays[k])
    torch.cuda.synchronize()
    for k in range(3):
        assert_same(outs[k][0].cpu().numpy(), ref["rgb"][2 * k:2 * k + 2], f"context {k}")
        assert_same(outs[k][1].cpu().numpy().view(np.uint32), ref["packed"][2 * k:2 * k + 2], f"context {k} packed")
        assert ctxs[k].stats()[0]["primary"] == V * H * W
        ctxs[k].close()
