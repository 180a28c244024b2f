"""rtx_query_closest / rtx_query_occluded on the GPU: rays and segments in device tensors, answers in device tensors, everything bit for bit
(NaN == NaN) against the batch oracle (orc.OracleScene.trace_closest with zero differentials: distance, point, normal, u / v and the three
ids as the RTX_AOV_*_ID channels number them; trace_any at seven maximum distances per ray):
  * the adversarial ray classes of tests/rayset.py over five scenes, through every kernel a flag selects;
  * a context with bounces == 0 and a frame without lights — what the debug hooks refuse (test_gpu_rays.traceable);
  * batch sizes around a wave and a packet, and a call of more than two internal rounds (RTX_QUERY_CHUNK_RAYS);
  * zero and NaN directions, channel subsets, nothing written past n;
  * the AOV channels of a ray view over the same rays, and the frames around a query unchanged;
  * a scene changed on the device (rtx_update_instances), stream order with torch, and every error code;
  * the unit-test hooks rtx_debug_trace_rays / rtx_debug_occluded, which run the queries' rounds from host arrays: the same answers as the
    queries, a queued frame left alone, rows that are no ray, more than one round."""
import copy
import ctypes as C

import numpy as np
import pytest

import rayset
import util
from test_gpu_rays import LANE_TRACE, PACKET_CLOSEST, chain_blas_scene, many_instances_scene, check_occ, traceable

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
FLAGS = {0: {}, LANE_TRACE: {"lane_trace": True}, PACKET_CLOSEST: {"packet_closest": True}}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def zero_diff(rays6):
    return np.concatenate([rays6, np.zeros((len(rays6), 12), f32)], axis=1).astype(f32)


def expected(o, rays6):
    """The oracle's answer per channel for rays with zero differentials."""
    hits, ids = o.trace_closest(zero_diff(rays6), threads=8)
    return {"distance": hits[:, 1].copy(), "position": hits[:, 2:5].copy(), "normal": hits[:, 5:8].copy(), "uv": hits[:, 9:11].copy(),
            "material_id": ids[:, 0].copy(), "object_id": ids[:, 1].copy(), "triangle_id": ids[:, 2].copy()}


def same_bits(got, want):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        eq = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        eq = got == want
    return eq.reshape(len(got), -1).all(axis=1)


def check_channels(got, want, labels=None, what=""):
    """Every channel of `got` (tensors or arrays) bit for bit; names the channels and the ray classes that differ."""
    bad = {}
    for name, g in got.items():
        g = host(g) if hasattr(g, "cpu") else g
        ok = same_bits(g, want[name][:len(g)])
        if not ok.all():
            rows = np.flatnonzero(~ok)
            bad[name] = (len(rows), rows[:6].tolist(), {} if labels is None else {str(c): int((labels[rows] == c).sum()) for c in np.unique(labels[rows])})
    assert not bad, (what, bad)


def segments_of(rays6, dist):
    """(n * k, 7): every ray at each of its k maximum distances."""
    n, k = dist.shape
    return np.concatenate([np.repeat(rays6, k, axis=0), dist.reshape(-1, 1)], axis=1).astype(f32)


SCENES = ["cube", "materials_aniso", "coincident", "chain_blas", "many_instances"]
_CACHE = {}


def load_scene(name):
    if name == "chain_blas":
        return chain_blas_scene()
    if name == "many_instances":
        return many_instances_scene()
    return util.load_golden(name)[0]


def generated(name, n=64, seed=21, strip=False):
    """(scene, rays (N, 6), distances (N, 7), labels, expected channels, expected occlusion (N, 7)), once per module run.
    strip: bounces 0 and no light at all."""
    key = (name, n, seed, strip)
    if key not in _CACHE:
        import orc
        from pyrtx import scene_io as sio
        sc = load_scene(name)
        if strip:
            sc = copy.deepcopy(sc)
            sc.config["bounces"] = 0
            sc.point_lights = np.zeros(0, sio.POINT_LIGHT); sc.spot_lights = np.zeros(0, sio.SPOT_LIGHT); sc.dir_lights = np.zeros(0, sio.DIR_LIGHT)
        o = orc.OracleScene(sc)
        rays18, dist3, labels, _ = rayset.generate(sc, n, seed, o)
        rays = np.ascontiguousarray(rays18[:, :6])
        dist = rayset.all_distances(dist3)
        _CACHE[key] = (sc, rays, dist, labels, expected(o, rays), o.trace_any(zero_diff(rays), dist))
    return _CACHE[key]


def check_scene(api, sc, rays, dist, labels, want, occ, what):
    r = api.Renderer(sc)
    rays_t = dev(rays)
    for flags, kw in FLAGS.items():
        got = r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), **kw)
        assert tuple(got) == tuple(api.QUERY_CHANNELS)
        check_channels(got, want, labels, f"{what} flags {flags}")
    seg_t = dev(segments_of(rays, dist))
    for flags in (0, LANE_TRACE):
        got = host(r.query_occluded(seg_t, **FLAGS[flags]))
        assert got.dtype == np.int32 and set(np.unique(got)) <= {0, 1}
        check_occ(got.reshape(dist.shape) != 0, occ, labels)
    return r


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_queries_equal_the_oracle(api, name):
    sc, rays, dist, labels, want, occ = generated(name)
    assert len(rays) <= 448
    check_scene(api, sc, rays, dist, labels, want, occ, name)


MISS27 = np.array([0.0, np.inf] + [0.0] * 25, f32)                  # the oracle's miss record: hit 0, distance inf, every other RayHit float 0


@pytest.mark.parametrize("name", ["materials_aniso", "cube"])
def test_the_debug_hooks_equal_the_queries(api, name):
    """rtx_debug_trace_rays with zero differentials against query_closest, column by channel, and rtx_debug_occluded against
    query_occluded, on one context: the same rounds, bit for bit.  The hook's material_id is 0 where the query's is -1 (a miss)."""
    sc, rays, dist, labels, want, occ = generated(name)
    assert len(rays) <= 448
    r = api.Renderer(traceable(sc))
    rays_t = dev(rays)
    for flags, kw in FLAGS.items():
        hook = r.debug_trace_rays(zero_diff(rays), flags)
        q = {k: host(v) for k, v in r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), **kw).items()}
        mat = np.where(q["material_id"] < 0, 0, q["material_id"]).astype(f32)
        cols = {"hit": (hook[:, 0], (q["object_id"] >= 0).astype(f32)), "distance": (hook[:, 1], q["distance"]), "point": (hook[:, 2:5], q["position"]),
                "normal": (hook[:, 5:8], q["normal"]), "material_id": (hook[:, 8], mat), "u, v": (hook[:, 9:11], q["uv"])}
        bad = {k: np.flatnonzero(~same_bits(g, w))[:6].tolist() for k, (g, w) in cols.items() if not same_bits(g, w).all()}
        assert not bad, (name, flags, bad)
    seg = segments_of(rays, dist)
    for flags in (0, LANE_TRACE):
        hook = r.debug_occluded(seg, flags)
        assert set(np.unique(hook)) <= {0, 1}
        assert np.array_equal(hook != 0, host(r.query_occluded(dev(seg), **FLAGS[flags])) != 0), (name, flags)


# ---- 2. no bounce level, no light ------------------------------------------------------------------------------------------------------
def test_queries_need_neither_a_bounce_level_nor_a_light(api):
    sc, rays, dist, labels, want, occ = generated("cube", strip=True)
    assert int(sc.config["bounces"][0]) == 0 and len(sc.point_lights) + len(sc.spot_lights) + len(sc.dir_lights) == 0
    r = check_scene(api, sc, rays, dist, labels, want, occ, "cube, bounces 0, no lights")
    with pytest.raises(api.RtxError):                                   # the debug hook on the same context: refused
        r.debug_trace_rays(zero_diff(rays))
    with pytest.raises(api.RtxError):
        r.debug_occluded(segments_of(rays, dist[:, :1]))


# ---- 3. batch sizes --------------------------------------------------------------------------------------------------------------------
def test_batch_sizes_around_a_wave_and_a_packet(api):
    """One 1025-ray set, its first n rays per call: ray i's answer does not depend on n."""
    sc, rays, dist, labels, want, occ = generated("materials_aniso", n=256, seed=22)
    assert len(rays) >= 1025
    pick = np.random.default_rng(3).permutation(len(rays))[:1025]
    rays, dist, occ = rays[pick], dist[pick, 1:2], occ[pick, 1:2]      # segments: exactly at the hit, the tie the strict < decides
    want = {k: v[pick] for k, v in want.items()}
    r = api.Renderer(sc)
    rays_t, seg_t = dev(rays), dev(segments_of(rays, dist))
    for n in (1, 63, 64, 65, 1023, 1024, 1025):
        for flags, kw in FLAGS.items():
            got = r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), n=n, **kw)
            assert all(len(t) == n for t in got.values())
            check_channels(got, want, None, f"n {n} flags {flags}")
        for flags in (0, LANE_TRACE):
            got = host(r.query_occluded(seg_t, n=n, **FLAGS[flags]))
            assert got.shape == (n,) and np.array_equal(got != 0, occ[:n, 0]), (n, flags)


# ---- 4. chunking -----------------------------------------------------------------------------------------------------------------------
def test_more_than_two_internal_rounds(api):
    """n = 2 * RTX_QUERY_CHUNK_RAYS + 1: three rounds, the last of one ray.  Built and compared on the device."""
    import torch
    sc, rays, dist, labels, want, occ = generated("materials_aniso", n=256, seed=22)
    pick = np.random.default_rng(4).integers(len(rays), size=4096)
    rays, d, occ = rays[pick], dist[pick, 1:2], occ[pick, 1]
    r = api.Renderer(sc)
    small_t, seg_small_t = dev(rays), dev(segments_of(rays, d))
    got = r.query_closest(small_t, ("distance", "triangle_id"))
    check_channels(got, {k: v[pick] for k, v in want.items()}, None, "the 4096-ray set")
    assert np.array_equal(host(r.query_occluded(seg_small_t)) != 0, occ)
    N = 2 * api.RTX_QUERY_CHUNK_RAYS + 1
    reps = (N + 4095) // 4096
    big = small_t.repeat(reps, 1)[:N]
    assert big.is_contiguous() and big.shape == (N, 6)
    out = r.query_closest(big, ("distance", "triangle_id"))
    assert tuple(out) == ("distance", "triangle_id")
    assert torch.equal(out["distance"].view(torch.int32), got["distance"].view(torch.int32).repeat(reps)[:N])
    assert torch.equal(out["triangle_id"], got["triangle_id"].repeat(reps)[:N])
    occ_big = r.query_occluded(seg_small_t.repeat(reps, 1)[:N])
    assert torch.equal(occ_big, dev(occ.astype(np.int32)).repeat(reps)[:N])


def test_more_than_one_round_through_a_hook(api):
    """n = RTX_QUERY_CHUNK_RAYS + 65: two rounds, the second ending in a partial packet.  Row i answers as row i mod len(rays) of a one-round call."""
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    r = api.Renderer(traceable(sc))
    rays18, seg = zero_diff(rays), segments_of(rays, dist[:, 1:2])
    small, small_occ = r.debug_trace_rays(rays18), r.debug_occluded(seg)
    assert np.array_equal(small_occ != 0, occ[:, 1])
    idx = np.arange(api.RTX_QUERY_CHUNK_RAYS + 65) % len(rays)
    big = r.debug_trace_rays(rays18[idx])
    assert big.shape == (len(idx), 27) and np.array_equal(big.view(np.uint32), small.view(np.uint32)[idx])
    assert np.array_equal(r.debug_occluded(seg[idx]), small_occ[idx])


# ---- 5. zero direction -----------------------------------------------------------------------------------------------------------------
def test_zero_direction_is_no_ray_and_nan_is_one(api):
    import orc
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    rays = rays.copy()
    hit = np.flatnonzero(np.isfinite(want["distance"]))
    rows = hit[[3, len(hit) // 2, len(hit) - 2]]                                             # rays that hit something: a miss value there is the rule, not the scene
    rays[rows[0], 3:6] = (0.0, 0.0, 0.0)
    rays[rows[1], 3:6] = (-0.0, 0.0, 0.0)
    rays[rows[2], 3:6] = (np.nan, 0.0, 0.0)
    o = orc.OracleScene(sc)
    ref = expected(o, rays)
    miss = {"distance": f32(np.inf), "position": 0.0, "normal": 0.0, "uv": 0.0, "material_id": -1, "object_id": -1, "triangle_id": -1}
    for row in rows[:2]:                                                # what the query must say for "no ray", whatever the oracle makes of a zero direction
        for k in ref:
            ref[k][row] = miss[k]
    untouched = np.setdiff1d(np.arange(len(rays)), rows)
    for k in ref:                                                       # the neighbours' expectations are those of the unedited set
        assert same_bits(ref[k][untouched], want[k][untouched]).all()
    r = api.Renderer(sc)
    d7 = np.full((len(rays), 1), np.inf, f32)
    seg = segments_of(rays, d7)
    occ_ref = o.trace_any(zero_diff(rays), d7)[:, 0]
    occ_ref[rows[:2]] = False                                           # a zero-direction segment is not occluded
    for flags, kw in FLAGS.items():
        check_channels(r.query_closest(dev(rays), tuple(api.QUERY_CHANNELS), **kw), ref, labels, f"flags {flags}")
    for flags in (0, LANE_TRACE):
        assert np.array_equal(host(r.query_occluded(dev(seg), **FLAGS[flags])) != 0, occ_ref), flags


def test_rows_that_are_no_ray_through_the_hooks(api):
    """Zero, NaN and infinite rows through rtx_debug_trace_rays / rtx_debug_occluded: the fill does not walk them (a NaN origin in the
    packet walk would never end), they answer as the miss record / not occluded, and their neighbours answer as without them."""
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    hit = np.flatnonzero(np.isfinite(want["distance"]))
    rows = hit[[3, len(hit) // 2, len(hit) - 2, 1, len(hit) // 3]]                           # rays that hit something
    assert len(set(rows.tolist())) == 5
    edited = rays.copy()
    edited[rows[0], 3:6] = (0.0, 0.0, 0.0)
    edited[rows[1], 3:6] = (-0.0, 0.0, 0.0)
    edited[rows[2], 3] = np.nan
    edited[rows[3], 1] = np.nan
    edited[rows[4], 2] = np.inf
    untouched = np.setdiff1d(np.arange(len(rays)), rows)
    r = api.Renderer(traceable(sc))
    d7 = np.full((len(rays), 1), np.inf, f32)
    for flags in FLAGS:
        base, got = r.debug_trace_rays(zero_diff(rays), flags), r.debug_trace_rays(zero_diff(edited), flags)
        assert (base[rows, 0] == 1.0).all(), flags
        assert np.array_equal(got[rows].view(np.uint32), np.tile(MISS27, (5, 1)).view(np.uint32)), (flags, got[rows, :3])
        assert np.array_equal(got[untouched].view(np.uint32), base[untouched].view(np.uint32)), flags
    for flags in (0, LANE_TRACE):
        base, got = r.debug_occluded(segments_of(rays, d7), flags), r.debug_occluded(segments_of(edited, d7), flags)
        assert (got[rows] == 0).all() and np.array_equal(got[untouched], base[untouched]), flags


# ---- 6. channel subsets and bounds -----------------------------------------------------------------------------------------------------
def test_channel_subsets_write_nothing_else(api):
    import torch
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    n, pad = len(rays), 64
    r = api.Renderer(sc)
    rays_t = dev(rays)

    def sentinels():
        out = {}
        for name, (_, dt, k) in api.QUERY_CHANNELS.items():
            shape = (n + pad, k) if k > 1 else (n + pad,)
            out[name] = torch.full(shape, -77.0, dtype=torch.float32, device="cuda") if dt == np.float32 else torch.full(shape, -77, dtype=torch.int32, device="cuda")
        return out

    def run(names, buffers):
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        got = r.query_closest(rays_t.data_ptr(), names, out={k: buffers[k].data_ptr() for k in names}, n=n)
        r.synchronize()
        return got

    full = sentinels()
    run(tuple(api.QUERY_CHANNELS), full)
    check_channels({k: t[:n] for k, t in full.items()}, want, labels, "all channels")
    for k, t in full.items():
        assert bool((t[n:] == -77).all()), f"{k}: rows past n were written"
    part = sentinels()
    run(("distance",), part)
    assert torch.equal(part["distance"][:n].view(torch.int32), full["distance"][:n].view(torch.int32))
    assert bool((part["distance"][n:] == -77).all())
    for k, t in part.items():
        if k != "distance":
            assert bool((t == -77).all()), f"{k} was not requested"
    # a bit without a pointer, and a pointer without its bit: neither is written (the C ABI's rule; the Python layer refuses both)
    both = sentinels()
    buf = api.RtxQueryBuffers()
    buf.distance = both["distance"].data_ptr(); buf.normal = both["normal"].data_ptr()
    torch.cuda.synchronize()
    assert r.lib.rtx_query_closest(r.ctx, rays_t.data_ptr(), n, api.RTX_QUERY_DISTANCE | api.RTX_QUERY_UV, C.byref(buf), 0) == 0
    r.synchronize()
    assert torch.equal(both["distance"][:n].view(torch.int32), full["distance"][:n].view(torch.int32))
    assert bool((both["normal"] == -77).all()) and bool((both["uv"] == -77).all())
    occ_t = torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")
    seg_t = dev(segments_of(rays, dist[:, 1:2]))
    torch.cuda.synchronize()
    r.query_occluded(seg_t.data_ptr(), out=occ_t.data_ptr(), n=n)
    r.synchronize()
    assert np.array_equal(host(occ_t[:n]) != 0, occ[:, 1]) and bool((occ_t[n:] == -77).all())


# ---- 7. agreement with the AOV path ----------------------------------------------------------------------------------------------------
def test_a_ray_view_with_aovs_says_the_same(api):
    """The pinhole rays of the golden's own camera through render_rays(aovs=...) and through query_closest: identical channels; the frame
    the ray view renders is the same before and after the query."""
    sc, _ = util.load_golden("materials_aniso")
    W, H = sc.width, sc.height
    rays18 = api.pinhole_rays(sc.camera[0], W, H)
    r = api.Renderer(sc)
    r.set_rays(rays18)
    aov = ("depth", "position", "normal", "uv", "material_id", "object_id", "triangle_id")
    before = r.render_rays(aovs=aov)
    got = r.query_closest(dev(rays18.reshape(-1, 18)[:, :6]), tuple(api.QUERY_CHANNELS))
    occ = r.query_occluded(dev(np.concatenate([rays18.reshape(-1, 18)[:, :6], np.full((W * H, 1), 1e30, f32)], axis=1)))
    after = r.render_rays(aovs=aov)
    for name, t in got.items():
        a = before["depth" if name == "distance" else name][0]
        assert same_bits(host(t), a.reshape((W * H,) + a.shape[2:])).all(), name
    import orc
    assert np.array_equal(host(occ) != 0, orc.OracleScene(sc).trace_any(rays18.reshape(-1, 18), np.full(W * H, 1e30, f32)))
    assert util.bit_exact(before["rgb"], after["rgb"]) and np.array_equal(before["packed"], after["packed"]) and before["stats"] == after["stats"]
    for name in aov:
        assert same_bits(before[name][0].reshape(W * H, -1), after[name][0].reshape(W * H, -1)).all(), name


def test_a_query_leaves_a_queued_frame_and_its_stats_alone(api):
    """render, query, read: the frame and rtx_get_stats are those of a context that made no query."""
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    r.render_async()
    got = r.query_closest(dev(rays), ("distance", "object_id"))
    r.query_occluded(dev(segments_of(rays, dist[:, :1])))
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    check_channels(got, want, labels)


def test_a_hook_call_leaves_a_queued_frame_and_its_stats_alone(api):
    """render, both debug hooks, read: the frame and rtx_get_stats are those of a context that made no hook call."""
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    sc = traceable(sc)
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    r.render_async()
    hits = r.debug_trace_rays(zero_diff(rays))
    blocked = r.debug_occluded(segments_of(rays, dist[:, :1]))
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    assert same_bits(hits[:, 1], want["distance"]).all() and np.array_equal(blocked != 0, occ[:, 0])


# ---- 8. device-side scene changes are seen ---------------------------------------------------------------------------------------------
def test_a_query_sees_the_instances_the_device_updated(api):
    import orc
    from test_gpu_update_instances import with_state
    from test_tlas_balanced_cpu import poses
    sc, _ = util.load_golden("tori16")
    r = api.Renderer(sc)
    pos, rot = poses("tori16", 3)
    p, q = dev(np.ascontiguousarray(pos, f32)), dev(np.ascontiguousarray(rot, f32))
    r.update_instances(p, q)
    moved = with_state(sc, r.read_frame_state())
    o = orc.OracleScene(moved)
    rays18, dist3, labels, _ = rayset.generate(moved, 64, 23, o)
    rays = np.ascontiguousarray(rays18[:, :6])
    want = expected(o, rays)
    old = expected(orc.OracleScene(sc), rays)
    assert not same_bits(want["distance"], old["distance"]).all(), "the poses moved nothing these rays see"
    for flags, kw in FLAGS.items():
        check_channels(r.query_closest(dev(rays), tuple(api.QUERY_CHANNELS), **kw), want, labels, f"flags {flags}")
    dist = rayset.all_distances(dist3)
    got = host(r.query_occluded(dev(segments_of(rays, dist))))
    check_occ(got.reshape(dist.shape) != 0, o.trace_any(zero_diff(rays), dist), labels)


# ---- 9. stream order -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["side", "default"])
def test_queries_are_ordered_on_torchs_stream(api, stream):
    """rays written by a torch op, the query, a torch reduction of its answer: one stream, nothing synchronised in between."""
    import torch
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    r = api.Renderer(sc)
    reps = 256                                                          # enough work that an unordered reader would run ahead of it
    src = dev(rays)
    hit = np.isfinite(want["distance"])
    want_res = (int(hit.sum()) * reps, int(want["triangle_id"].astype(np.int64).sum()) * reps, int(occ[:, 5].sum()) * reps)
    ctx = torch.cuda.stream(torch.cuda.Stream()) if stream == "side" else torch.cuda.stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    with ctx:
        big = torch.empty((len(rays) * reps, 6), dtype=torch.float32, device="cuda")
        big.copy_(src.repeat(reps, 1))                                  # the write the query must wait for
        got = r.query_closest(big, ("distance", "triangle_id"))
        n_hits = torch.isfinite(got["distance"]).sum()
        tri_sum = got["triangle_id"].to(torch.int64).sum()
        seg = torch.cat([big, torch.zeros((len(big), 1), dtype=torch.float32, device="cuda")], dim=1)
        seg[:, 6] = float(rayset.FIXED_DIST[2])                         # 1e30, column 5 of rayset.all_distances: written in stream order too
        n_occ = r.query_occluded(seg).sum()
        res = (int(n_hits), int(tri_sum), int(n_occ))                   # the first wait
    assert res == want_res


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------------
def test_every_error_code_and_a_valid_query_after_it(api):
    import torch
    sc, rays, dist, labels, want, occ = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(rays)
    rays_t, seg_t = dev(rays), dev(segments_of(rays, dist[:, :1]))
    dist_t = torch.full((n,), -77.0, dtype=torch.float32, device="cuda")
    occ_t = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    buf = api.RtxQueryBuffers(); buf.distance = dist_t.data_ptr()
    rp, sp, op, D = rays_t.data_ptr(), seg_t.data_ptr(), occ_t.data_ptr(), api.RTX_QUERY_DISTANCE
    torch.cuda.synchronize()
    closest = [((r.ctx, rp, 0, D, C.byref(buf), 0), INVALID), ((r.ctx, rp, -5, D, C.byref(buf), 0), INVALID),      # n < 1
               ((r.ctx, None, n, D, C.byref(buf), 0), INVALID),                                                 # NULL rays
               ((r.ctx, rp, n, D, None, 0), INVALID),                                                           # NULL out
               ((r.ctx, rp, n, D | 8, C.byref(buf), 0), INVALID), ((r.ctx, rp, n, 256, C.byref(buf), 0), INVALID),   # bits outside RTX_QUERY_ALL (8 = albedo)
               ((r.ctx, rp, n, 0, C.byref(buf), 0), INVALID),                                                   # no channel
               ((r.ctx, rp, n, D, C.byref(buf), 1), INVALID), ((r.ctx, rp, n, D, C.byref(buf), 128), INVALID),   # flags other than lane / packet-closest
               ((None, rp, n, D, C.byref(buf), 0), INVALID)]
    for args, code in closest:
        assert lib.rtx_query_closest(*args) == code, args[2:]
    occluded = [((r.ctx, sp, 0, op, 0), INVALID), ((r.ctx, None, n, op, 0), INVALID), ((r.ctx, sp, n, None, 0), INVALID),
                ((r.ctx, sp, n, op, 8), INVALID), ((None, sp, n, op, 0), INVALID)]
    for args, code in occluded:
        assert lib.rtx_query_occluded(*args) == code, args[2:]
    r.synchronize()
    assert bool((dist_t == -77).all()) and bool((occ_t == -77).all()), "an error queued something"
    # RTX_ERR_STATE: before rtx_set_frame, and in heat-map mode; RTX_ERR_LIMIT: the stack rule of a render call
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_closest(empty.ctx, rp, n, D, C.byref(buf), 0) == STATE
    assert lib.rtx_query_occluded(empty.ctx, sp, n, op, 0) == STATE
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert lib.rtx_query_closest(rh.ctx, rp, n, D, C.byref(buf), 0) == STATE
    assert lib.rtx_query_occluded(rh.ctx, sp, n, op, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert lib.rtx_query_closest(rs.ctx, rp, n, D, C.byref(buf), 0) == LIMIT
    assert lib.rtx_query_occluded(rs.ctx, sp, n, op, 0) == LIMIT
    for other in (empty, rh, rs):
        other.synchronize()
    assert bool((dist_t == -77).all()) and bool((occ_t == -77).all()), "an error queued something"
    # ... and the context that refused all of the above still answers
    check_channels(r.query_closest(rays_t, tuple(api.QUERY_CHANNELS)), want, labels, "after the errors")
    assert np.array_equal(host(r.query_occluded(seg_t)) != 0, occ[:, 0])
