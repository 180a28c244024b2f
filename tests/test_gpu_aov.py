"""Per-pixel primary-hit AOVs (include/rtx.h rtx_bind_aovs / rtx_read_aovs, RTX_RENDER_AOV).

Every channel is what Raytracer::bounce has for the pixel's primary ray: depth must equal the oracle's `dist` output bit for bit, the
hit fields must equal orc_trace_closest on the primary ray rebuilt with the oracle's render_tile arithmetic, the albedo Material::diffuse x
Texture::sample of the oracle (or its Sky::sample on a miss), and the ids must be the oracle's winner (orc_trace_closest_ids) and name a
primitive the ray hits at that depth.  The colour,
packed pixels and ray counts of an AOV call must equal the call without it in every launch shape.
"""
import ctypes as C

import numpy as np
import pytest

import util
from test_gpu_parity import MODES          # every launch shape rtx_render_tiles knows
from test_gpu_views import SCENE_VIEW, camera_set, with_camera

pytestmark = pytest.mark.gpu

f32 = np.float32
ALL = ("depth", "position", "normal", "albedo", "uv", "material_id", "object_id", "triangle_id")
IDS = ("material_id", "object_id", "triangle_id")
SCENES = ["cube", "materials_aniso", "materials_ewa", "materials_bilinear", "monkey_small", "tori16", "dynamic", "ragged", "coincident"]


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
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.int32)


def assert_same(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ"


def primary_rays(sc):
    """(H*W, 18) float32 primary rays of Raytracer::render_tile as the oracle evaluates them (rt_oracle.c render_tile: unfused
    multiply and add, correctly rounded sqrt and divide): origin, direction, dO_dx = dO_dy = 0, dD_dx, dD_dy."""
    cam = sc.camera[0]
    ax, ay, tl = (np.asarray(cam[k], f32) for k in ("rotated_x_axis", "rotated_y_axis", "rotated_top_left_corner"))
    j, i = np.meshgrid(np.arange(sc.height, dtype=f32), np.arange(sc.width, dtype=f32), indexing="ij")
    i = i.reshape(-1, 1); j = j.reshape(-1, 1)
    d = ax * i + (ay * j + tl)                                               # vmadd_s(ax, is, vmadd_s(ay, js, tl))
    dot = lambda a, b: a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
    dd = dot(d, d)
    inv = f32(1.0) / np.sqrt(dd)
    denom = inv / dd
    axb = np.broadcast_to(ax, d.shape); ayb = np.broadcast_to(ay, d.shape)
    dDx = (ax * dd[:, None] - d * dot(d, axb)[:, None]) * denom[:, None]
    dDy = (ay * dd[:, None] - d * dot(d, ayb)[:, None]) * denom[:, None]
    rays = np.zeros((d.shape[0], 18), f32)
    rays[:, 0:3] = np.asarray(cam["position"], f32)
    rays[:, 3:6] = d * inv[:, None]
    rays[:, 12:15] = dDx; rays[:, 15:18] = dDy
    return rays


_ORACLE = {}


def oracle(name, sc):
    """dist of orc render (want_dist) and, per pixel, orc_trace_closest_ids of the primary ray (hit fields and the winner's material,
    object and triangle ids), the oracle's albedo and sky colour."""
    if name in _ORACLE:
        return _ORACLE[name]
    import orc
    o = orc.OracleScene(sc); L = orc.lib()
    dist = o.render(threads=8, want_dist=True)["dist"].reshape(-1)
    rays = primary_rays(sc)
    hits, ids = o.trace_closest(rays)
    albedo = np.zeros((len(rays), 3), f32)
    cfg = sc.config
    mode, filt, aniso = int(cfg["texture_mode"][0]), int(cfg["mip_filter"][0]), float(cfg["max_anisotropy"][0])
    diff = mode == 2                                                         # RAY_DIFFERENTIALS_ENABLED with mipmapping (Config.h:46)
    tex = np.zeros(3, f32)
    for p in range(len(rays)):
        r = rays[p]
        h = hits[p]
        if h[0] > 0:
            m = sc.materials[int(h[8])]
            a = np.asarray(m["diffuse"], f32)
            if int(m["texture_id"]) >= 0:
                dv = [float(x) for x in h[11:15]] if diff else [0.0] * 4
                L.orc_texture_sample(C.byref(o._tex[int(m["texture_id"])]), mode, filt, aniso, float(h[9]), float(h[10]), *dv, tex.ctypes.data)
                a = a * tex
            albedo[p] = a
        else:
            d = np.ascontiguousarray(r[3:6])
            L.orc_sky_sample(o._sky.ctypes.data, o.struct.sky_size, d.ctypes.data, albedo[p].ctypes.data)
    _ORACLE[name] = (dist, rays, hits, albedo, ids)
    return _ORACLE[name]


def flat(out, name):
    a = out[name]
    return a.reshape(a.shape[0] * a.shape[1], -1) if a.ndim == 3 else a.reshape(-1)


# ---- 2 + 3: depth and hit fields against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_channels_match_the_oracle(api, name):
    sc = load(name)
    out = api.Renderer(sc).render_aovs(ALL)
    H, W = sc.height, sc.width
    for ch, shape in (("depth", (H, W)), ("position", (H, W, 3)), ("normal", (H, W, 3)), ("albedo", (H, W, 3)), ("uv", (H, W, 2)),
                      ("material_id", (H, W)), ("object_id", (H, W)), ("triangle_id", (H, W))):
        assert out[ch].shape == shape, ch
    dist, rays, hits, albedo, ids = oracle(name, sc)
    # the rebuilt primary rays are the oracle's: orc_trace_closest finds the distance its own render reports, +inf on a miss
    assert_same(hits[:, 1], dist, "orc_trace_closest distance vs oracle render dist")
    assert_same(flat(out, "depth"), dist, "depth")
    hit = hits[:, 0] > 0
    assert hit.any()
    assert np.isinf(flat(out, "depth")[~hit]).all()
    assert_same(flat(out, "position")[hit], hits[hit, 2:5], "position")
    assert_same(flat(out, "normal")[hit], hits[hit, 5:8], "normal")
    assert_same(flat(out, "uv")[hit], hits[hit, 9:11], "uv")
    assert_same(flat(out, "material_id")[hit], hits[hit, 8].astype(np.int32), "material_id")
    assert_same(flat(out, "albedo"), albedo, "albedo")
    for ch in ("position", "normal", "uv"):
        assert not flat(out, ch)[~hit].any(), ch
    for ch in IDS:
        assert (flat(out, ch)[~hit] == -1).all(), ch
    # the winner itself, not merely a primitive at that depth: a coplanar neighbour or a coincident instance is a different id
    for k, ch in enumerate(IDS):
        assert_same(flat(out, ch), ids[:, k], ch)
    check_ids(sc, out, rays)


# ---- 4: ids --------------------------------------------------------------------------------------------------------------------------
def check_ids(sc, out, rays):
    depth = flat(out, "depth").astype(np.float64)
    mat, obj, tri = flat(out, "material_id"), flat(out, "object_id"), flat(out, "triangle_id")
    ni, ns = len(sc.instances), len(sc.spheres)
    hit = np.isfinite(depth)
    assert ((obj >= 0) == hit).all()
    o = rays[:, 0:3].astype(np.float64); d = rays[:, 3:6].astype(np.float64)
    is_tri = hit & (obj < ni)
    assert ((tri >= 0) == is_tri).all(), "triangle_id is set exactly for triangle hits"
    for p in np.nonzero(is_tri)[0]:
        inst = sc.instances[obj[p]]
        b = sc.blas[int(inst["blas_id"])]
        cold, hot = b.tri_cold[tri[p]], b.tri_hot[tri[p]]
        assert int(cold["material_id"]) + b.material_offset == mat[p]
        M = np.asarray(inst["world_inv"], np.float64).reshape(4, 4)            # row r = cells[4r .. 4r+3] (rtx_math.h xform_pos)
        ro = M[:3, :3] @ o[p] + M[:3, 3]; rd = M[:3, :3] @ d[p]
        p0 = np.asarray(hot["position_0"], np.float64); e1 = np.asarray(hot["position_edge_1"], np.float64); e2 = np.asarray(hot["position_edge_2"], np.float64)
        h = np.cross(rd, e2); a = e1 @ h; s = ro - p0; q = np.cross(s, e1)
        t = (e2 @ q) / a
        assert abs(t - depth[p]) <= 1e-4 * abs(depth[p]), (p, t, depth[p])
    for p in np.nonzero(hit & (obj >= ni) & (obj < ni + ns))[0]:
        sp = sc.spheres[obj[p] - ni]
        x = o[p] + d[p] * depth[p] - np.asarray(sp["center"], np.float64)
        assert int(sp["material_id"]) == mat[p]
        assert abs(np.sqrt(x @ x) - np.sqrt(float(sp["radius_squared"]))) <= 1e-4 * max(1.0, depth[p]), p
    for p in np.nonzero(hit & (obj >= ni + ns))[0]:
        pl = sc.planes[obj[p] - ni - ns]
        x = o[p] + d[p] * depth[p]
        assert int(pl["material_id"]) == mat[p]
        assert abs(np.asarray(pl["normal"], np.float64) @ x + float(pl["distance"])) <= 1e-4 * max(1.0, depth[p]), p


# ---- 1 + 4: colour untouched, ids equal in every launch shape --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES) + ["count_work"])
@pytest.mark.parametrize("name", ["materials_aniso", "tori16", "ragged"])
def test_colour_untouched_and_channels_equal_in_every_launch_shape(api, name, mode):
    flags = MODES.get(mode, {"count_work": True})
    sc = load(name)
    r = api.Renderer(sc)
    plain = r.render(**flags)
    out = r.render_aovs(ALL, **flags)
    assert_same(out["rgb"], plain["rgb"], "rgb"); assert_same(out["packed"], plain["packed"], "packed")
    assert out["stats"] == plain["stats"]
    if mode == "count_work":
        assert out["work"] == plain["work"]
    ref = api.Renderer(sc).render_aovs(ALL)
    for ch in ALL:
        assert_same(out[ch], ref[ch], ch)


# ---- 5: views ------------------------------------------------------------------------------------------------------------------------
def single_view_aovs(api, sc, cams, **flags):
    r = api.Renderer(sc)
    outs = []
    for k in range(len(cams)):
        r.set_frame(with_camera(sc, cams[k]))
        outs.append(r.render_aovs(ALL, **flags))
    return outs


@pytest.mark.parametrize("name", ["materials_aniso", "tori16", "dynamic", "ragged"])
def test_views_equal_single_view_renders(api, name, monkeypatch):
    if name == "ragged":
        monkeypatch.setenv("RTX_SLOT_BUDGET", str(1024 * 15 * 5))       # 4 x 3 tiles per view, 5 tiles per batch: batches straddle views
    sc = load(name)
    cams = camera_set(sc)
    singles = single_view_aovs(api, sc, cams)
    r = api.Renderer(sc)
    r.set_views(cams)
    out = r.render_views(aovs=ALL)
    for k, s in enumerate(singles):
        assert_same(out["rgb"][k], s["rgb"], f"view {k} rgb")
        for ch in ALL:
            assert_same(out[ch][k], s[ch], f"view {k} {ch}")
    assert len({out["depth"][k].tobytes() for k in range(len(cams))}) == len(cams)
    part = r.render_views(2, 3, aovs=("depth", "object_id"), serial=True)     # a sub-range; the pixel index is view * W * H + y * W + x
    for k in range(3):
        assert_same(part["depth"][k], singles[2 + k]["depth"], f"view {2 + k} depth")
        assert_same(part["object_id"][k], singles[2 + k]["object_id"], f"view {2 + k} object_id")
    one = api.Renderer(sc); one.set_views(cams[SCENE_VIEW:SCENE_VIEW + 1])
    single = one.render_views(aovs=IDS)
    tiles = api.Renderer(sc).render_aovs(IDS)
    for ch in IDS:
        assert_same(single[ch][0], tiles[ch], ch)



# ---- 6: partial and clipped work --------------------------------------------------------------------------------------------------
def device_buffers(torch, pixels, fill=True):
    from pyrtx.ctypes_structs import AOV_CHANNELS
    bufs = {}
    for ch in ALL:
        _, dt, k = AOV_CHANNELS[ch]
        shape = (pixels, k) if k > 1 else (pixels,)
        bufs[ch] = (torch.full(shape, -7.25, dtype=torch.float32, device="cuda") if dt == np.float32
                    else torch.full(shape, -77, dtype=torch.int32, device="cuda"))
    return bufs


def host(bufs):
    return {ch: t.cpu().numpy() for ch, t in bufs.items()}


def test_strided_tiles_and_ragged_edges_write_only_rendered_pixels(api):
    import torch
    sc = load("ragged")
    W, H = sc.width, sc.height
    full = api.Renderer(sc).render_aovs(ALL)
    r = api.Renderer(sc)
    extra = 4096
    bufs = device_buffers(torch, W * H + extra)
    torch.cuda.synchronize()
    r.bind_aovs(ALL, {ch: t.data_ptr() for ch, t in bufs.items()}, W * H + extra)
    r.render_async(first_tile=1, tile_stride=3, tile_count=4, aov=True)
    r.synchronize()
    got = host(bufs)
    tcx = (W + 31) // 32
    mask = np.zeros((H, W), bool)
    for t in range(1, 12, 3):
        x, y = (t % tcx) * 32, (t // tcx) * 32
        mask[y:y + 32, x:x + 32] = True
    m = mask.reshape(-1)
    for ch in ALL:
        g = got[ch]
        want = full[ch].reshape(W * H, -1) if full[ch].ndim == 3 else full[ch].reshape(-1)
        assert_same(g[:W * H][m], want[m], ch)
        sentinel = g[:W * H][~m]
        assert (bits(sentinel) == bits(np.full_like(sentinel, -7.25 if g.dtype == np.float32 else -77))).all(), ch
        tail = g[W * H:]
        assert (bits(tail) == bits(np.full_like(tail, -7.25 if g.dtype == np.float32 else -77))).all(), f"{ch}: written past W*H"


# ---- 7: bindings and errors --------------------------------------------------------------------------------------------------------
def test_bindings_rebinds_and_unbound_channels(api):
    import torch
    sc = load("materials_aniso")
    W, H = sc.width, sc.height
    r = api.Renderer(sc)
    own = r.render_aovs(ALL)
    a = device_buffers(torch, W * H); b = device_buffers(torch, W * H)
    torch.cuda.synchronize()
    # caller buffers == own buffers; a bound channel with a NULL pointer and unbound channels are not written
    r.bind_aovs(("depth", "normal", "triangle_id"), {"depth": a["depth"].data_ptr(), "normal": a["normal"].data_ptr(),
                                                      "uv": a["uv"].data_ptr(), "albedo": a["albedo"].data_ptr()}, W * H)
    r.render_async(aov=True)
    r.synchronize()
    # rebind between calls: the next call writes the new buffers only
    r.bind_aovs(ALL, {ch: t.data_ptr() for ch, t in b.items()}, W * H)
    r.render_async(aov=True, serial=True)
    r.synchronize()
    ga, gb = host(a), host(b)
    for ch in ("depth", "normal"):
        assert_same(ga[ch].reshape(own[ch].shape), own[ch], ch)
    for ch in ("position", "albedo", "uv", "material_id", "object_id", "triangle_id"):
        fill = -7.25 if ga[ch].dtype == np.float32 else -77
        assert (bits(ga[ch]) == bits(np.full_like(ga[ch], fill))).all(), f"{ch} written although not bound"
    for ch in ALL:
        assert_same(gb[ch].reshape(own[ch].shape), own[ch], ch)
    # a plain call after unbinding writes nothing and renders as before
    r.bind_aovs(0)
    plain = r.render()
    assert_same(plain["rgb"], own["rgb"], "rgb")
    assert_same(host(b)["depth"], gb["depth"], "depth after unbind")


def test_error_cases(api):
    import torch
    sc = load("materials_aniso")
    W, H = sc.width, sc.height
    r = api.Renderer(sc)
    lib, ctx = r.lib, r.ctx
    assert lib.rtx_render_tiles(ctx, 0, 1, sc.tile_count, api.RTX_RENDER_AOV) == 5            # nothing bound: RTX_ERR_STATE
    r.set_views(camera_set(sc)[:2])
    assert lib.rtx_render_views(ctx, 0, 2, api.RTX_RENDER_AOV) == 5
    assert lib.rtx_bind_aovs(ctx, 256, None, 0) == 1                                           # unknown bit
    t = torch.zeros(W * H * 2 - 1, dtype=torch.float32, device="cuda")
    from pyrtx.ctypes_structs import RtxAovBuffers
    dev = RtxAovBuffers(); dev.depth = t.data_ptr()
    assert lib.rtx_bind_aovs(ctx, 1, C.byref(dev), 0) == 1                                     # caller buffers without capacity
    assert lib.rtx_bind_aovs(ctx, 1, C.byref(dev), W * H * 2 - 1) == 0
    assert lib.rtx_render_tiles(ctx, 0, 1, sc.tile_count, api.RTX_RENDER_AOV) == 0
    assert lib.rtx_render_views(ctx, 0, 1, api.RTX_RENDER_AOV) == 0
    assert lib.rtx_render_views(ctx, 0, 2, api.RTX_RENDER_AOV) == 1                            # 2 * W * H pixels > capacity
    assert lib.rtx_render_views(ctx, 1, 1, api.RTX_RENDER_AOV) == 1
    host_bufs = RtxAovBuffers(); d = np.zeros(W * H, f32); host_bufs.depth = d.ctypes.data
    assert lib.rtx_read_aovs(ctx, 0, 1, C.byref(host_bufs)) == 5                                # caller buffers bound
    assert lib.rtx_debug_group_loopback(ctx, 2, api.RTX_RENDER_AOV) == 1                        # the group path refuses AOVs
    r.bind_aovs("depth")
    assert lib.rtx_read_aovs(ctx, 0, 1, C.byref(host_bufs)) == 1                                # own buffer never written yet
    r.synchronize()
    heat = util.load_golden("materials_heat")[0]
    rh = api.Renderer(heat)
    rh.bind_aovs(ALL)
    assert rh.lib.rtx_render_tiles(rh.ctx, 0, 1, heat.tile_count, api.RTX_RENDER_AOV) == 5     # heat-map mode
    assert rh.lib.rtx_render_tiles(rh.ctx, 0, 1, heat.tile_count, 0) == 0


# ---- 7: hipGraph replay and the fused shading kernel ---------------------------------------------------------------------------------
def test_graph_replay_alternating_calls_and_rebinds(api, monkeypatch):
    import torch
    monkeypatch.setenv("RTX_GRAPH", "1")
    sc = load("tori16")
    W, H = sc.width, sc.height
    ref_r = api.Renderer(sc)
    plain_ref = ref_r.render()
    ref = ref_r.render_aovs(ALL)
    r = api.Renderer(sc)
    a = device_buffers(torch, W * H); b = device_buffers(torch, W * H)
    torch.cuda.synchronize()
    # three identical calls = eager, captured, replayed; the graph of one binding must not be replayed after a rebind (a a a -> b)
    seq = ["a", "a", "a", "b", "b", "b", "a", "plain", "plain", "plain", "a", "a", "b", "plain"]
    for k, step in enumerate(seq):
        if step == "plain":
            out = r.render()
        else:
            bufs = a if step == "a" else b
            for t in bufs.values():
                t.fill_(-1)
            torch.cuda.synchronize()
            r.bind_aovs(ALL, {ch: t.data_ptr() for ch, t in bufs.items()}, W * H)
            r.render_async(aov=True)
            out = {"stats": r.stats()[0]}
            out["rgb"], out["packed"] = r.framebuffer()
            got = host(bufs)
            for ch in ALL:
                assert_same(got[ch].reshape(ref[ch].shape), ref[ch], f"call {k} ({step}): {ch}")
        assert_same(out["rgb"], plain_ref["rgb"], f"call {k}: rgb")
        assert out["stats"] == plain_ref["stats"]


def test_fused_shading_gives_the_same_channels(api, monkeypatch):
    sc = load("materials_aniso")
    ref = api.Renderer(sc).render_aovs(ALL)
    monkeypatch.setenv("RTX_FUSE_SHADE", "1")
    r = api.Renderer(sc)
    plain = r.render()
    out = r.render_aovs(ALL)
    assert_same(out["rgb"], plain["rgb"], "rgb") ; assert out["stats"] == plain["stats"]
    for ch in ALL + ("rgb", "packed"):
        assert_same(out[ch], ref[ch], ch)
    cams = camera_set(sc)[:3]
    r.set_views(cams)
    v = r.render_views(aovs=ALL)
    for k in range(3):
        s = api.Renderer(with_camera(sc, cams[k])).render_aovs(ALL)
        for ch in ALL:
            assert_same(v[ch][k], s[ch], f"view {k} {ch}")


# ---- 8: torch --------------------------------------------------------------------------------------------------------------------
def test_render_views_into_with_aovs_on_torch_streams(api):
    import torch
    sc = load("ragged")
    W, H = sc.width, sc.height
    cams = camera_set(sc)
    V = len(cams)
    r = api.Renderer(sc)
    r.set_views(cams)
    ref = r.render_views(aovs=ALL)
    from pyrtx.ctypes_structs import AOV_CHANNELS
    for own_stream in (False, True):
        rgb = torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"); packed = torch.zeros((V, H, W), dtype=torch.int32, device="cuda")
        aovs = {ch: torch.full(api.aov_shape(ch, V, H, W), -3, dtype=torch.float32 if AOV_CHANNELS[ch][1] == np.float32 else torch.int32, device="cuda")
                for ch in ALL}
        torch.cuda.synchronize()
        s = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            r.render_views_into(rgb, packed, aovs=aovs)
            copies = {ch: t.clone() for ch, t in aovs.items()}                 # queued after the render on the same stream
        torch.cuda.synchronize()
        assert_same(rgb.cpu().numpy(), ref["rgb"], "rgb")
        for ch in ALL:
            assert_same(copies[ch].cpu().numpy(), ref[ch], f"{ch} (own stream: {own_stream})")
