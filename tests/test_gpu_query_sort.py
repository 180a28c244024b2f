"""RTX_QUERY_SORT on the GPU (Renderer.query_closest / query_occluded with sort=True, Renderer.debug_query_order):
  * the order the device sorts a round into is host.query_sort_order's, exactly, around a wave, a packet and a workgroup, for rays and segments;
  * every channel and the occlusion bit with sort=True, bit for bit against the batch oracle (the helpers of test_gpu_query.py), over the
    rayset classes with dead rows planted, through every kernel a flag selects, with channel subsets and sentinels behind row n - 1;
  * a call of two internal rounds; a sorted call between render calls and unsorted calls on a caller's stream; a second sorted call
    allocates nothing; the error codes."""
import ctypes as C

import numpy as np
import pytest

import rayset
from test_gpu_query import (FLAGS, INVALID, STATE, LANE_TRACE, api, check_channels, dev, generated, host, same_bits, segments_of)      # noqa: F401 (api: the fixture)

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (1, 63, 64, 65, 257, 4097)
MISS = {"distance": f32(np.inf), "position": 0.0, "normal": 0.0, "uv": 0.0, "material_id": -1, "object_id": -1, "triangle_id": -1}
_SETS = {}


def shuffled_set(name, n=4097, seed=41):
    """(scene, rays (n, 6), expected channels, segments (n, 7), expected occlusion (n,)): the rayset rows of test_gpu_query.generated(name)
    drawn n times in a seeded order, every 11th row made dead (zero direction, NaN or infinite component), once per module run."""
    key = (name, n, seed)
    if key not in _SETS:
        sc, rays, dist, labels, want, occ = generated(name)
        rng = np.random.default_rng(seed)
        pick = rng.integers(len(rays), size=n)
        col = rng.integers(dist.shape[1], size=n)
        rays = rays[pick].copy()
        want = {k: v[pick].copy() for k, v in want.items()}
        seg_d, occ = dist[pick, col].copy(), occ[pick, col].copy()
        dead = np.arange(5, n, 11)
        for j, row in enumerate(dead):
            if j % 3 == 0:
                rays[row, 3:6] = (0.0, -0.0, 0.0)
            elif j % 3 == 1:
                rays[row, rng.integers(6)] = np.nan
            else:
                rays[row, rng.integers(6)] = np.inf if j % 2 else -np.inf
        for k in want:
            want[k][dead] = MISS[k]
        occ[dead] = False
        nan_dist = np.arange(9, n, 37)                                  # a NaN maximum distance: never occluded, not walked
        seg_d[nan_dist] = np.nan; occ[nan_dist] = False
        seg = np.concatenate([rays, seg_d.reshape(-1, 1)], axis=1).astype(f32)
        _SETS[key] = (sc, np.ascontiguousarray(rays), want, seg, occ)
    return _SETS[key]


# ---- 1. the order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [6, 7])
def test_device_order_is_the_hosts(api, width):
    from pyrtx import host as h
    sc, rays, want, seg, occ = shuffled_set("cube")
    rows = rays if width == 6 else seg
    r = api.Renderer(sc)
    rows_t = dev(rows)
    for n in SIZES:
        got = host(r.debug_query_order(rows_t, n=n))
        ref = h.query_sort_order(rows[:n])
        assert got.dtype == np.int32 and got.shape == (n,)
        assert np.array_equal(got, ref), (width, n, np.flatnonzero(got != ref)[:8].tolist())
    # hostile origins: an extent that overflows fp32, and a round whose live rows are all equal
    far = rows[:257].copy(); far[:, :3] = np.random.default_rng(3).choice(np.array([3e38, -3e38, 3.4028235e38, 0.0, -0.0], f32), size=(257, 3))
    same = np.tile(rows[0], (257, 1)); same[::9, 3:6] = 0.0
    for name, hostile in (("far", far), ("same", same)):
        assert np.array_equal(host(r.debug_query_order(dev(hostile))), h.query_sort_order(hostile)), (width, name)


# ---- 2. the answers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "coincident", "many_instances"])
def test_sorted_answers_equal_the_oracle(api, name):
    sc, rays, want, seg, occ = shuffled_set(name)
    r = api.Renderer(sc)
    rays_t, seg_t = dev(rays), dev(seg)
    for n in SIZES:
        for flags, kw in FLAGS.items():
            got = r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), n=n, sort=True, **kw)
            assert tuple(got) == tuple(api.QUERY_CHANNELS) and all(len(t) == n for t in got.values())
            check_channels(got, want, None, f"{name} n {n} flags {flags} sorted")
        for flags in (0, LANE_TRACE):
            got = host(r.query_occluded(seg_t, n=n, sort=True, **FLAGS[flags]))
            assert got.dtype == np.int32 and got.shape == (n,) and set(np.unique(got)) <= {0, 1}
            assert np.array_equal(got != 0, occ[:n]), (name, n, flags, np.flatnonzero((got != 0) != occ[:n])[:8].tolist())
    # and the call without the flag says the same, bit for bit
    plain = r.query_closest(rays_t, tuple(api.QUERY_CHANNELS))
    check_channels(r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), sort=True), {k: host(v) for k, v in plain.items()}, None, f"{name} sorted against unsorted")


def test_sorted_channel_subsets_write_nothing_else(api):
    import torch
    sc, rays, want, seg, occ = shuffled_set("cube")
    n, pad = 257, 64
    r = api.Renderer(sc)
    rays_t, seg_t = dev(rays), dev(seg)

    def sentinels():
        out = {}
        for name, (_, dt, k) in api.QUERY_CHANNELS.items():
            shape = (n + pad, k) if k > 1 else (n + pad,)
            out[name] = torch.full(shape, -77.0, dtype=torch.float32, device="cuda") if dt == np.float32 else torch.full(shape, -77, dtype=torch.int32, device="cuda")
        return out

    for names in (tuple(api.QUERY_CHANNELS), ("distance",), ("normal", "object_id"), ("uv", "material_id", "triangle_id")):
        buffers = sentinels()
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        r.query_closest(rays_t.data_ptr(), names, out={k: buffers[k].data_ptr() for k in names}, n=n, sort=True)
        r.synchronize()
        check_channels({k: buffers[k][:n] for k in names}, want, None, f"subset {names}")
        for k, t in buffers.items():
            assert bool((t[n:] == -77).all()), f"{k}: rows past n were written"
            if k not in names:
                assert bool((t == -77).all()), f"{k} was not requested"
    occ_t = torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.query_occluded(seg_t.data_ptr(), out=occ_t.data_ptr(), n=n, sort=True)
    r.synchronize()
    assert np.array_equal(host(occ_t[:n]) != 0, occ[:n]) and bool((occ_t[n:] == -77).all())


# ---- 3. two rounds ---------------------------------------------------------------------------------------------------------------------
def test_two_internal_rounds(api):
    """n = RTX_QUERY_CHUNK_RAYS + 65, shuffled: the 4097-row set (checked against the oracle) drawn in a random order on the device."""
    import torch
    from pyrtx import host as h
    sc, rays, want, seg, occ = shuffled_set("cube")
    r = api.Renderer(sc)
    names = ("distance", "normal", "triangle_id")
    small_t, seg_small_t = dev(rays), dev(seg)
    small = r.query_closest(small_t, names, sort=True)
    check_channels(small, want, None, "the 4097-row set")
    N = api.RTX_QUERY_CHUNK_RAYS + 65
    idx = torch.randint(len(rays), (N,), generator=torch.Generator(device="cuda").manual_seed(7), device="cuda")
    big = small_t[idx].contiguous()
    out = r.query_closest(big, names, sort=True)
    for k in names:
        assert torch.equal(out[k].view(torch.int32), small[k][idx].view(torch.int32)), k
    occ_big = r.query_occluded(seg_small_t[idx].contiguous(), sort=True)
    assert torch.equal(occ_big, dev(occ.astype(np.int32))[idx])
    order = r.debug_query_order(big)                                    # every round a permutation of its own rows; the second is the host's
    first = torch.sort(order[:api.RTX_QUERY_CHUNK_RAYS]).values
    assert torch.equal(first, torch.arange(api.RTX_QUERY_CHUNK_RAYS, dtype=torch.int32, device="cuda"))
    tail = host(big[api.RTX_QUERY_CHUNK_RAYS:])
    assert np.array_equal(host(order[api.RTX_QUERY_CHUNK_RAYS:]), api.RTX_QUERY_CHUNK_RAYS + h.query_sort_order(tail))


# ---- 4. stream order -------------------------------------------------------------------------------------------------------------------
def test_a_sorted_call_between_render_calls_and_unsorted_calls_on_a_callers_stream(api):
    import torch
    import util
    sc, rays, want, seg, occ = shuffled_set("cube")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    names = tuple(api.QUERY_CHANNELS)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        rays_t = torch.empty((len(rays), 6), dtype=torch.float32, device="cuda")
        rays_t.copy_(dev(rays))                                         # the write every query below must wait for
        seg_t = dev(seg)
        before = r.query_closest(rays_t, names)
        occ_before = r.query_occluded(seg_t)
        r.render_async()
        sorted_ = r.query_closest(rays_t, names, sort=True)
        occ_sorted = r.query_occluded(seg_t, sort=True)
        order = r.debug_query_order(rays_t)
        r.render_async()
        after = r.query_closest(rays_t, names)
        occ_after = r.query_occluded(seg_t)
        stats, _ = r.stats()                                            # the first wait
        rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    for what, got in (("before", before), ("sorted", sorted_), ("after", after)):
        check_channels(got, want, None, what)
    for got in (occ_before, occ_sorted, occ_after):
        assert np.array_equal(host(got) != 0, occ)
    assert np.array_equal(np.sort(host(order)), np.arange(len(rays)))


# ---- 5. allocation ---------------------------------------------------------------------------------------------------------------------
def test_a_second_sorted_call_allocates_nothing(api):
    """Free device memory (hipMemGetInfo) is the same before and after a sorted call of a size the context has sorted before.  The figure is
    the device's, so another process may move it: three calls are measured and one without a change is the observation — a call that
    allocated would lower it every time."""
    import torch
    sc, rays, want, seg, occ = shuffled_set("cube")
    r = api.Renderer(sc)
    n = len(rays)
    rays_t, seg_t = dev(rays), dev(seg)
    out = {"distance": torch.empty((n,), dtype=torch.float32, device="cuda")}
    occ_t = torch.empty((n,), dtype=torch.int32, device="cuda")
    r.query_closest(rays_t, ("distance",), out=out)                     # the queues, by an unsorted call
    r.query_closest(rays_t, ("distance",), out=out, sort=True)          # the sort scratch, by the first sorted call
    r.query_occluded(seg_t, out=occ_t, sort=True)
    torch.cuda.synchronize()
    changes = []
    for _ in range(3):
        free0 = torch.cuda.mem_get_info()[0]
        r.query_closest(rays_t, ("distance",), out=out, sort=True)
        r.query_occluded(seg_t, out=occ_t, sort=True)
        r.debug_query_order(rays_t, n=n - 1)                            # a smaller n: nothing either (its result comes from torch's cache or not: measured apart)
        torch.cuda.synchronize()
        changes.append(free0 - torch.cuda.mem_get_info()[0])
    assert 0 in changes[1:], changes                                    # the first round may fill torch's cache for the order tensor
    check_channels(out, want, None, "after the repeated calls")
    assert np.array_equal(host(occ_t) != 0, occ)


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def test_error_codes_of_the_sort_flag_and_the_order_hook(api):
    import torch
    sc, rays, want, seg, occ = shuffled_set("cube")
    n = 257
    r = api.Renderer(sc)
    lib = r.lib
    rays_t, seg_t = dev(rays[:n]), dev(seg[:n])
    dist_t = torch.full((n,), -77.0, dtype=torch.float32, device="cuda")
    occ_t = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    order_t = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    buf = api.RtxQueryBuffers(); buf.distance = dist_t.data_ptr()
    rp, sp, op, dp, D, S = rays_t.data_ptr(), seg_t.data_ptr(), occ_t.data_ptr(), order_t.data_ptr(), api.RTX_QUERY_DISTANCE, api.RTX_QUERY_SORT
    torch.cuda.synchronize()
    assert S == 256
    for bad in (S | 1, S | 8, S | 128, S | 512):
        assert lib.rtx_query_closest(r.ctx, rp, n, D, C.byref(buf), bad) == INVALID, bad
        assert lib.rtx_query_occluded(r.ctx, sp, n, op, bad) == INVALID, bad
    for rf in (5, 0, 8, -6):
        assert lib.rtx_debug_query_order(r.ctx, rp, rf, n, dp) == INVALID, rf
    assert lib.rtx_debug_query_order(r.ctx, None, 6, n, dp) == INVALID
    assert lib.rtx_debug_query_order(r.ctx, rp, 6, n, None) == INVALID
    assert lib.rtx_debug_query_order(r.ctx, rp, 6, 0, dp) == INVALID
    assert lib.rtx_debug_query_order(None, rp, 6, n, dp) == INVALID
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_closest(empty.ctx, rp, n, D, C.byref(buf), S) == STATE
    assert lib.rtx_query_occluded(empty.ctx, sp, n, op, S) == STATE
    assert lib.rtx_debug_query_order(empty.ctx, rp, 6, n, dp) == STATE
    assert lib.rtx_debug_query_order(empty.ctx, rp, 5, n, dp) == STATE      # the query calls' checks come first
    r.synchronize(); empty.synchronize()
    assert bool((dist_t == -77).all()) and bool((occ_t == -77).all()) and bool((order_t == -77).all()), "an error queued something"
    # the flag with each of the two kernel flags, through the C ABI, on the context that refused all of the above
    for fl in (S, S | api.RTX_RENDER_LANE_TRACE, S | api.RTX_RENDER_PACKET_CLOSEST):
        assert lib.rtx_query_closest(r.ctx, rp, n, D, C.byref(buf), fl) == 0, fl
        r.synchronize()
        assert same_bits(host(dist_t), want["distance"][:n]).all(), fl
        dist_t.fill_(-77.0); torch.cuda.synchronize()
    assert lib.rtx_query_occluded(r.ctx, sp, n, op, S | api.RTX_RENDER_LANE_TRACE) == 0
    r.synchronize()
    assert np.array_equal(host(occ_t) != 0, occ[:n])
