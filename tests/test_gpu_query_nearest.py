"""rtx_query_nearest on the GPU: points in device tensors, answers in device tensors, every channel bit for bit (NaN == NaN) against the host
twin (host.query_nearest, the same code of csrc/rtx_nearest_math.h) run on the arrays read back from the context:
  * the point classes of tests/pointset.py and their critical maximum distances over five scenes, one of them with a stack that goes past
    RTX_LDS_STACK into the spill, one with a deep TLAS;
  * batch sizes around a wave and a workgroup, one call that crosses a round, channel subsets, guard elements, out= tensors, raw pointers;
  * sort=True: identical answers row for row with dead rows planted, and the order itself against host.query_sort_order;
  * after update_instances with random unit quaternions, after build_blas and refit_blas;
  * a context with bounces 0 and no lights; the frames and rtx_get_stats around a query unchanged; stream order with torch;
  * every error code in the documented order, the stack rule's RTX_ERR_LIMIT among them (refused by the host: nothing runs near an overflow)."""
import copy
import ctypes as C

import numpy as np
import pytest

import pointset
import util
from test_gpu_query import check_channels, dev, host as to_host, same_bits
from test_gpu_rays import chain_blas_scene, many_instances_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
SCENES = ["cube", "coincident", "materials_aniso", "chain_blas", "many_instances"]
_CACHE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def load_scene(name):
    if name == "chain_blas":
        return chain_blas_scene()
    if name == "many_instances":
        return many_instances_scene()
    return util.load_golden(name)[0]


def read_back(r, sc):
    """What the context holds, as host.query_nearest takes it."""
    inst, nodes, idx = r.read_frame_state()
    return (inst, nodes, idx, sc.spheres, sc.planes), [r.read_blas(b) for b in range(len(sc.blas))]


def twin(r, sc, pts, channels=None):
    from pyrtx import host
    state, blas = read_back(r, sc)
    out = host.query_nearest(state, pts, channels or tuple(r_channels()), blas=blas)
    out.pop("stack_max")
    return out


def r_channels():
    from pyrtx import api
    return api.QUERY_CHANNELS


def generated(name, n=180, seed=31):
    """(scene, points (N <= 448, 4), labels padded with -1 for the distance rows, host answers from the scene's own arrays), once per run."""
    key = (name, n, seed)
    if key not in _CACHE:
        from pyrtx import host
        sc = load_scene(name)
        pts, lab = pointset.generate(sc, n, seed)
        d0 = host.query_nearest(sc, pts, "distance")["distance"]
        keep = np.flatnonzero(np.isfinite(d0))[:: max(1, len(pts) // 12)][:12]
        allp = np.concatenate([pts, pointset.distance_rows(pts[keep], d0[keep])])[:448]
        labels = np.concatenate([lab, np.full(len(allp) - len(lab), -1)])[:448]
        want = host.query_nearest(sc, allp, tuple(r_channels()))
        _CACHE[key] = (sc, np.ascontiguousarray(allp), labels, want)
    return _CACHE[key]


# ---- 1. parity with the host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_host_walk(api, name):
    from pyrtx import host
    sc, pts, labels, want = generated(name)
    assert len(pts) <= 448
    if name == "chain_blas":
        assert want["stack_max"] > 16, "this scene is here to reach the spill region"          # RTX_LDS_STACK
    r = api.Renderer(sc)
    got = r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS))
    assert tuple(got) == tuple(api.QUERY_CHANNELS)
    check_channels(got, want, labels, name)
    check_channels(got, twin(r, sc, pts), labels, f"{name}, arrays read back")
    assert np.isfinite(to_host(got["distance"])).sum() > len(pts) // 3
    check_channels(r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS), sort=True), want, labels, f"{name} sorted")


def test_bounces_zero_and_no_lights(api):
    from pyrtx import scene_io as sio
    sc, pts, labels, want = generated("cube")
    sc = copy.deepcopy(sc)
    sc.config["bounces"] = 0
    sc.point_lights = np.zeros(0, sio.POINT_LIGHT); sc.spot_lights = np.zeros(0, sio.SPOT_LIGHT); sc.dir_lights = np.zeros(0, sio.DIR_LIGHT)
    r = api.Renderer(sc)
    check_channels(r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS)), want, labels, "bounces 0, no lights")


# ---- 2. batch sizes and rounds ---------------------------------------------------------------------------------------------------------
def test_batch_sizes_around_a_wave_and_a_workgroup(api):
    sc, pts, labels, want = generated("materials_aniso")
    assert len(pts) >= 257
    r = api.Renderer(sc)
    pts_t = dev(pts)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for sort in (False, True):
            got = r.query_nearest(pts_t, tuple(api.QUERY_CHANNELS), n=n, sort=sort)
            assert all(len(t) == n for t in got.values())
            check_channels(got, want, None, f"n {n} sort {sort}")


def test_one_call_crosses_a_round(api):
    import torch
    sc, pts, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    small = dev(pts)
    got = r.query_nearest(small, ("distance", "triangle_id", "position"))
    N = api.RTX_QUERY_CHUNK_RAYS + 65
    reps = (N + len(pts) - 1) // len(pts)
    big = small.repeat(reps, 1)[:N].contiguous()
    for sort in (False, True):
        out = r.query_nearest(big, ("distance", "triangle_id", "position"), sort=sort)
        assert torch.equal(out["distance"].view(torch.int32), got["distance"].view(torch.int32).repeat(reps)[:N]), sort
        assert torch.equal(out["triangle_id"], got["triangle_id"].repeat(reps)[:N]), sort
        assert torch.equal(out["position"].view(torch.int32), got["position"].view(torch.int32).repeat(reps, 1)[:N]), sort


# ---- 3. channel subsets, guards, out= and raw pointers ---------------------------------------------------------------------------------
def test_channel_subsets_write_nothing_else(api):
    import torch
    sc, pts, labels, want = generated("materials_aniso")
    n, pad = len(pts), 64
    r = api.Renderer(sc)
    pts_t = dev(pts)

    def sentinels():
        out = {}
        for name, (_, dt, k) in api.QUERY_CHANNELS.items():
            shape = (n + pad, k) if k > 1 else (n + pad,)
            out[name] = torch.full(shape, -77.0, dtype=torch.float32, device="cuda") if dt == np.float32 else torch.full(shape, -77, dtype=torch.int32, device="cuda")
        return out

    def run(names, buffers, sort=False):
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        r.query_nearest(pts_t.data_ptr(), names, out={k: buffers[k].data_ptr() for k in names}, n=n, sort=sort)
        r.synchronize()

    for sort in (False, True):
        full = sentinels()
        run(tuple(api.QUERY_CHANNELS), full, sort)
        check_channels({k: t[:n] for k, t in full.items()}, want, labels, f"all channels, raw pointers, sort {sort}")
        for k, t in full.items():
            assert bool((t[n:] == -77).all()), f"{k}: rows past n were written"
    for names in (("distance",), ("position",), ("normal", "uv"), ("material_id",), ("object_id", "triangle_id")):
        part = sentinels()
        run(names, part)
        for k, t in part.items():
            if k in names:
                assert same_bits(to_host(t[:n]), want[k]).all() and bool((t[n:] == -77).all()), (names, k)
            else:
                assert bool((t == -77).all()), f"{k} was not requested with {names}"
    # a bit without a pointer, and a pointer without its bit: neither is written
    both = sentinels()
    buf = api.RtxQueryBuffers()
    buf.distance = both["distance"].data_ptr(); buf.normal = both["normal"].data_ptr()
    torch.cuda.synchronize()
    assert r.lib.rtx_query_nearest(r.ctx, pts_t.data_ptr(), n, api.RTX_QUERY_DISTANCE | api.RTX_QUERY_UV, C.byref(buf), 0) == 0
    r.synchronize()
    assert same_bits(to_host(both["distance"][:n]), want["distance"]).all()
    assert bool((both["normal"] == -77).all()) and bool((both["uv"] == -77).all())
    # out= tensors are the ones returned
    mine = {"distance": torch.empty((n,), dtype=torch.float32, device="cuda"), "normal": torch.empty((n, 3), dtype=torch.float32, device="cuda")}
    got = r.query_nearest(pts_t, ("distance", "normal", "object_id"), out=mine)
    assert got["distance"] is mine["distance"] and got["normal"] is mine["normal"] and got["object_id"].shape == (n,)
    check_channels(got, want, labels, "out= tensors")


# ---- 4. sorted rounds ------------------------------------------------------------------------------------------------------------------
def test_sorted_rounds_answer_row_for_row_and_in_the_hosts_order(api):
    from pyrtx import host
    sc, pts, labels, want = generated("coincident")
    rng = np.random.default_rng(8)
    pts = pts[rng.permutation(len(pts))].copy()
    pts[::6, 3] = rng.choice(np.array([0.0, -2.0, np.nan], f32), size=len(pts[::6]))          # planted dead rows
    pts[2::11, 0] = np.nan
    r = api.Renderer(sc)
    t = dev(pts)
    plain = r.query_nearest(t, tuple(api.QUERY_CHANNELS))
    srt = r.query_nearest(t, tuple(api.QUERY_CHANNELS), sort=True)
    ref = twin(r, sc, pts)
    check_channels(plain, ref, None, "unsorted")
    check_channels(srt, ref, None, "sorted")
    dead = ~(np.isfinite(pts[:, :3]).all(axis=1) & (pts[:, 3] > 0))
    assert dead.sum() > 20 and np.isinf(to_host(srt["distance"])[dead]).all() and (to_host(srt["object_id"])[dead] == -1).all()
    order = to_host(r.debug_query_order(t))
    assert np.array_equal(order, host.query_sort_order(pts))
    assert dead[order[len(pts) - int(dead.sum()):]].all()


# ---- 5. device-side scene changes ------------------------------------------------------------------------------------------------------
def test_after_update_instances_with_random_unit_quaternions(api):
    from test_gpu_update_instances import with_state
    sc, _ = util.load_golden("tori16")
    r = api.Renderer(sc)
    n = len(sc.instances)
    rng = np.random.default_rng(41)
    pos = (rng.uniform(-1, 1, (n, 3)) * np.array([8.0, 4.0, 6.0]) + np.array([0.0, 3.0, 10.0])).astype(f32)
    q = rng.normal(size=(n, 4)); rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    p_t, q_t = dev(pos), dev(rot)
    before = r.query_nearest(dev(pointset.generate(sc, 64, 3)[0]), ("distance",))
    r.update_instances(p_t, q_t)
    moved = with_state(sc, r.read_frame_state())
    pts, labels = pointset.generate(moved, 150, seed=42)
    pts = pts[:448]
    got = r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS))
    check_channels(got, twin(r, sc, pts), labels[:448], "after update_instances")
    check_channels(r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS), sort=True), twin(r, sc, pts), labels[:448], "after update_instances, sorted")
    old = api.Renderer(sc).query_nearest(dev(pts), ("distance",))
    assert not same_bits(to_host(old["distance"]), to_host(got["distance"])).all(), "the poses moved nothing these points see"
    assert before["distance"].shape[0] > 0


def test_after_build_blas_and_refit_blas(api):
    from test_gpu_blas_build import base_scene, build_on_device, deform, twin_of
    from test_tlas_balanced_cpu import poses
    from test_gpu_update_instances import with_state
    sc = base_scene()
    r = api.Renderer(sc)
    keep = build_on_device(r, "padded")                              # Torus with every fifth triangle invalid: NaN pad slots in the leaves
    pos, rot = poses("tori16", 1)
    p, q = dev(pos), dev(rot)
    r.update_instances(p, q)
    state = with_state(sc, r.read_frame_state()); state.blas = [r.read_blas(0)]
    pts, labels = pointset.generate(state, 120, seed=51)
    pts = pts[:448]
    got = r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS))
    check_channels(got, twin(r, sc, pts), labels[:448], "after build_blas")
    assert np.isfinite(to_host(got["distance"])).sum() > len(pts) // 3
    verts = twin_of("padded")[3]
    moved = dev(deform(verts, "wave", seed=21))
    r.refit_blas(0, moved)
    r.update_instances(p, q)
    after = r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS), sort=True)
    check_channels(after, twin(r, sc, pts), labels[:448], "after refit_blas")
    assert not same_bits(to_host(after["distance"]), to_host(got["distance"])).all(), "the refit moved nothing these points see"
    del keep


# ---- 6. the frames around a query ------------------------------------------------------------------------------------------------------
def test_a_query_leaves_frames_and_stats_alone(api):
    sc, pts, labels, want = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    first = r.render()
    r.render_async()
    got = r.query_nearest(dev(pts), tuple(api.QUERY_CHANNELS), sort=True)
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    after = r.render()
    for out in (first, after):
        assert out["stats"] == ref["stats"] and util.bit_exact(out["rgb"], ref["rgb"]) and np.array_equal(out["packed"], ref["packed"])
    check_channels(got, want, labels)


# ---- 7. stream order -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["side", "default"])
def test_queries_are_ordered_on_torchs_stream(api, stream):
    """points written by a torch op, the query, a torch reduction of its answer: one stream, nothing synchronised in between."""
    import torch
    sc, pts, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    reps = 256
    src = dev(pts)
    hit = np.isfinite(want["distance"])
    want_res = (int(hit.sum()) * reps, int(want["triangle_id"].astype(np.int64).sum()) * reps)
    ctx = torch.cuda.stream(torch.cuda.Stream()) if stream == "side" else torch.cuda.stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    with ctx:
        big = torch.empty((len(pts) * reps, 4), dtype=torch.float32, device="cuda")
        big.copy_(src.repeat(reps, 1))                                  # the write the query must wait for
        got = r.query_nearest(big, ("distance", "triangle_id"))
        res = (int(torch.isfinite(got["distance"]).sum()), int(got["triangle_id"].to(torch.int64).sum()))      # the first wait
    assert res == want_res


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_every_error_code_in_order_and_a_valid_query_after_it(api):
    import torch
    sc, pts, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(pts)
    pts_t = dev(pts)
    dist_t = torch.full((n,), -77.0, dtype=torch.float32, device="cuda")
    buf = api.RtxQueryBuffers(); buf.distance = dist_t.data_ptr()
    pp, D, B = pts_t.data_ptr(), api.RTX_QUERY_DISTANCE, C.byref(buf)
    torch.cuda.synchronize()
    cases = [((r.ctx, pp, 0, D, B, 0), INVALID), ((r.ctx, pp, -5, D, B, 0), INVALID), ((r.ctx, None, n, D, B, 0), INVALID), ((r.ctx, pp, n, D, None, 0), INVALID),
             ((r.ctx, pp, n, D | 8, B, 0), INVALID), ((r.ctx, pp, n, 256, B, 0), INVALID), ((r.ctx, pp, n, 0, B, 0), INVALID),
             ((r.ctx, pp, n, D, B, 1), INVALID), ((r.ctx, pp, n, D, B, 16), INVALID), ((r.ctx, pp, n, D, B, 64 | 256), INVALID),      # the ray kernels' flags are not this call's
             ((None, pp, n, D, B, 0), INVALID)]
    for args, code in cases:
        assert lib.rtx_query_nearest(*args) == code, args[2:]
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_nearest(empty.ctx, pp, n, D, B, 0) == STATE
    assert lib.rtx_query_nearest(empty.ctx, pp, n, 0, B, 0) == INVALID            # the argument checks come first
    assert lib.rtx_query_nearest(empty.ctx, pp, n, D, B, 1) == INVALID
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert lib.rtx_query_nearest(rh.ctx, pp, n, D, B, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert lib.rtx_query_nearest(rs.ctx, pp, n, D, B, 0) == LIMIT                 # the stack rule of a render call
    # the walk's own rule: the chain mesh has its deepest inner node at depth 22 (24 entries for a ray walk) under a TLAS of one leaf: the
    # ordered descent needs (-1 + 1) + (22 + 1) = 23, so stack_size 24 serves rays and points; a TLAS with inner nodes over it does not
    chain = chain_blas_scene(); chain.config["stack_size"] = 24
    rc = api.Renderer(chain)
    assert lib.rtx_query_nearest(rc.ctx, pp, n, D, B, 0) == 0
    three = copy.deepcopy(chain)                                               # three instances: a TLAS whose deepest inner node is at depth 1
    three.instances = np.concatenate([chain.instances] * 3)
    root = chain.blas[0].nodes[0]
    boxes, centres = [], []
    for k in range(3):
        three.instances["world"][k][3] += 9.0 * k; three.instances["world_inv"][k][3] -= 9.0 * k
        boxes.append(np.concatenate([root["aabb_min"] + (9 * k, 0, 0), root["aabb_max"] + (9 * k, 0, 0)])); centres.append((9.0 * k, 0, 0))
    from pyrtx import host
    three.tlas_nodes, three.tlas_indices = host.tlas_build_balanced(np.array(centres, f32), np.array(boxes, f32))
    assert host.tlas_balanced_inner_depth(3) == 1
    rt = api.Renderer(three)
    rt.render()                                                                # rays are served: 22 + 2 entries
    assert lib.rtx_query_nearest(rt.ctx, pp, n, D, B, 0) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    # a frame with a scaled instance: RTX_ERR_STATE after the checks of a render call (a shallow stack stays RTX_ERR_LIMIT) and before the walk's
    # own stack rule (the three chains, enlarged by 2, are no longer RTX_ERR_LIMIT); the argument checks still come first; nothing is queued
    import affineset
    rn = api.Renderer(affineset.with_linear(three, [affineset.LINEAR["uniform2"]]))
    rsn = api.Renderer(affineset.with_linear(shallow, [affineset.LINEAR["uniform2"]]))
    assert lib.rtx_query_nearest(rn.ctx, pp, n, D, B, 0) == STATE and "rigid" in lib.rtx_last_error(rn.ctx).decode()
    assert lib.rtx_query_nearest(rn.ctx, pp, n, 0, B, 0) == INVALID and lib.rtx_query_nearest(rsn.ctx, pp, n, D, B, 0) == LIMIT
    rn.synchronize(); rsn.synchronize()
    for other in (empty, rh, rs, rc, rt):
        other.synchronize()
    r.synchronize()
    assert "stack" in lib.rtx_last_error(rt.ctx).decode()
    check_channels(r.query_nearest(pts_t, tuple(api.QUERY_CHANNELS)), want, labels, "after the errors")
