"""rtx_query_sweep on the GPU: rows in device tensors, answers in device tensors, every channel bit for bit (NaN == NaN) against the host twin
(host.query_sweep, the same code of csrc/rtx_sweep_math.h) run on the scene's arrays and on the arrays read back from the context:
  * the row classes of tests/sweepset.py and their critical D over five scenes, one of them with a stack that goes past RTX_LDS_STACK into
    the spill, one with a deep TLAS;
  * batch sizes around a wave and a workgroup, one call that crosses a round, channel subsets, guard elements, out= tensors, raw pointers;
  * sort=True: identical answers row for row on shuffled rows with dead rows planted;
  * after update_instances with random unit quaternions, after build_blas and refit_blas;
  * a context with bounces 0 and no lights; the frames and rtx_get_stats around a query unchanged; stream order with torch;
  * every error code in the documented order, the stack rule's RTX_ERR_LIMIT among them (refused by the host: nothing runs near an overflow)."""
import copy
import ctypes as C

import numpy as np
import pytest

import sweepset
import util
from test_gpu_query import check_channels, dev, host as to_host, same_bits
from test_gpu_query_nearest import load_scene, read_back
from test_gpu_rays import chain_blas_scene

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


def twin(r, sc, rows, channels=None):
    from pyrtx import api, host
    state, blas = read_back(r, sc)
    out = host.query_sweep(state, rows, channels or tuple(api.QUERY_CHANNELS), blas=blas)
    out.pop("stack_max")
    return out


def generated(name, n=224, seed=31):
    """(scene, rows (N <= 448, 8), labels padded with -1 for the critical-D rows, host answers from the scene's own arrays), once per run."""
    key = (name, n, seed)
    if key not in _CACHE:
        from pyrtx import api, host
        sc = load_scene(name)
        rows, lab = sweepset.generate(sc, n, seed)
        t0 = host.query_sweep(sc, rows, "distance")["distance"]
        keep = np.flatnonzero(np.isfinite(t0) & (t0 > 0))[:: max(1, len(rows) // 12)][:12]
        allr = np.concatenate([rows, sweepset.bound_rows(rows[keep], t0[keep])])[:448]
        labels = np.concatenate([lab, np.full(len(allr) - len(lab), -1)])[:448]
        want = host.query_sweep(sc, allr, tuple(api.QUERY_CHANNELS))
        _CACHE[key] = (sc, np.ascontiguousarray(allr), labels, want)
    return _CACHE[key]


# ---- 1. parity with the host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_host_walk(api, name):
    sc, rows, labels, want = generated(name)
    assert len(rows) <= 448
    if name == "chain_blas":
        assert want["stack_max"] > 16, "this scene is here to reach the spill region"          # RTX_LDS_STACK
    r = api.Renderer(sc)
    got = r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS))
    assert tuple(got) == tuple(api.QUERY_CHANNELS)
    check_channels(got, want, labels, name)
    check_channels(got, twin(r, sc, rows), labels, f"{name}, arrays read back")
    t = to_host(got["distance"])
    assert np.isfinite(t).sum() > len(rows) // 3 and (t == 0).any() and (np.isfinite(t) & (t > 0)).any()
    check_channels(r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS), sort=True), want, labels, f"{name} sorted")


def test_bounces_zero_and_no_lights(api):
    from pyrtx import scene_io as sio
    sc, rows, labels, want = generated("cube")
    sc = copy.deepcopy(sc)
    sc.config["bounces"] = 0
    sc.point_lights = np.zeros(0, sio.POINT_LIGHT); sc.spot_lights = np.zeros(0, sio.SPOT_LIGHT); sc.dir_lights = np.zeros(0, sio.DIR_LIGHT)
    r = api.Renderer(sc)
    check_channels(r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS)), want, labels, "bounces 0, no lights")


# ---- 2. batch sizes and rounds ---------------------------------------------------------------------------------------------------------
def test_batch_sizes_around_a_wave_and_a_workgroup(api):
    sc, rows, labels, want = generated("materials_aniso")
    assert len(rows) >= 257
    r = api.Renderer(sc)
    rows_t = dev(rows)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for sort in (False, True):
            got = r.query_sweep(rows_t, tuple(api.QUERY_CHANNELS), n=n, sort=sort)
            assert all(len(t) == n for t in got.values())
            check_channels(got, want, None, f"n {n} sort {sort}")


def test_one_call_crosses_a_round(api):
    """2^20 + 3 rows, mostly misses and dead rows: the scene's rows once, then rows that leave the scene and rows with a zero direction."""
    import torch
    sc, rows, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    N = api.RTX_QUERY_CHUNK_RAYS + 3
    assert N == 2 ** 20 + 3
    fill = np.zeros((2, 8), f32); fill[0] = [0, 1e4, 0, 0, 1, 0, 5.0, 0.01]; fill[1] = [0, 0, 0, 0, 0, 0, 1.0, 0.01]      # far above everything, moving up; dead
    from pyrtx import host
    assert np.isinf(host.query_sweep(sc, fill, "distance")["distance"]).all()
    big = torch.empty((N, 8), dtype=torch.float32, device="cuda")
    big[:] = dev(fill).repeat((N + 1) // 2, 1)[:N]
    small = dev(rows)
    k = len(rows)
    big[:k] = small; big[N - k:] = small                                # real rows at the start of round 0 and at the end of round 1
    ref = r.query_sweep(small, ("distance", "triangle_id", "position"))
    check_channels(ref, want, labels, "the small call")
    for sort in (False, True):
        out = r.query_sweep(big, ("distance", "triangle_id", "position"), sort=sort)
        for name in ref:
            assert torch.equal(out[name][:k].view(torch.int32), ref[name].view(torch.int32)) and torch.equal(out[name][N - k:].view(torch.int32), ref[name].view(torch.int32)), (sort, name)
        mid = slice(k, N - k)
        assert bool(torch.isinf(out["distance"][mid]).all()) and bool((out["triangle_id"][mid] == -1).all()) and not bool(out["position"][mid].any())


# ---- 3. channel subsets, guards, out= and raw pointers ---------------------------------------------------------------------------------
def test_channel_subsets_write_nothing_else(api):
    import torch
    sc, rows, labels, want = generated("materials_aniso")
    n, pad = len(rows), 64
    r = api.Renderer(sc)
    rows_t = dev(rows)

    def sentinels():
        out = {}
        for name, (_, dt, k) in api.QUERY_CHANNELS.items():
            shape = (n + pad, k) if k > 1 else (n + pad,)
            out[name] = torch.full(shape, -77.0, dtype=torch.float32, device="cuda") if dt == np.float32 else torch.full(shape, -77, dtype=torch.int32, device="cuda")
        return out

    def run(names, buffers, sort=False):
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        r.query_sweep(rows_t.data_ptr(), names, out={k: buffers[k].data_ptr() for k in names}, n=n, sort=sort)
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
    assert r.lib.rtx_query_sweep(r.ctx, rows_t.data_ptr(), n, api.RTX_QUERY_DISTANCE | api.RTX_QUERY_UV, C.byref(buf), 0) == 0
    r.synchronize()
    assert same_bits(to_host(both["distance"][:n]), want["distance"]).all()
    assert bool((both["normal"] == -77).all()) and bool((both["uv"] == -77).all())
    # out= tensors are the ones returned
    mine = {"distance": torch.empty((n,), dtype=torch.float32, device="cuda"), "normal": torch.empty((n, 3), dtype=torch.float32, device="cuda")}
    got = r.query_sweep(rows_t, ("distance", "normal", "object_id"), out=mine)
    assert got["distance"] is mine["distance"] and got["normal"] is mine["normal"] and got["object_id"].shape == (n,)
    check_channels(got, want, labels, "out= tensors")


# ---- 4. sorted rounds ------------------------------------------------------------------------------------------------------------------
def test_sorted_rounds_answer_row_for_row_on_shuffled_rows(api):
    sc, rows, labels, want = generated("coincident")
    rng = np.random.default_rng(8)
    rows = rows[rng.permutation(len(rows))].copy()
    rows[::6, 7] = rng.choice(np.array([0.0, -2.0, np.nan, np.inf], f32), size=len(rows[::6]))          # planted dead rows: the key does not see the radius
    rows[2::11, 0] = np.nan
    r = api.Renderer(sc)
    t = dev(rows)
    plain = r.query_sweep(t, tuple(api.QUERY_CHANNELS))
    srt = r.query_sweep(t, tuple(api.QUERY_CHANNELS), sort=True)
    ref = twin(r, sc, rows)
    check_channels(plain, ref, None, "unsorted")
    check_channels(srt, ref, None, "sorted")
    dead = ~sweepset.is_live(rows)
    assert dead.sum() > 20 and np.isinf(to_host(srt["distance"])[dead]).all() and (to_host(srt["object_id"])[dead] == -1).all()
    # the hooks that expose the order keep their widths
    buf = dev(np.zeros(len(rows), np.int32))
    assert r.lib.rtx_debug_query_order(r.ctx, t.data_ptr(), 8, len(rows), buf.data_ptr()) == INVALID


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
    r.update_instances(p_t, q_t)
    moved = with_state(sc, r.read_frame_state())
    rows, labels = sweepset.generate(moved, 150, seed=42)
    rows = rows[:448]
    got = r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS))
    check_channels(got, twin(r, sc, rows), labels[:448], "after update_instances")
    check_channels(r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS), sort=True), twin(r, sc, rows), labels[:448], "after update_instances, sorted")
    old = api.Renderer(sc).query_sweep(dev(rows), ("distance",))
    assert not same_bits(to_host(old["distance"]), to_host(got["distance"])).all(), "the poses moved nothing these rows see"


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
    rows, labels = sweepset.generate(state, 120, seed=51)
    rows = rows[:448]
    got = r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS))
    check_channels(got, twin(r, sc, rows), labels[:448], "after build_blas")
    assert np.isfinite(to_host(got["distance"])).sum() > len(rows) // 3
    verts = twin_of("padded")[3]
    moved = dev(deform(verts, "wave", seed=21))
    r.refit_blas(0, moved)
    r.update_instances(p, q)
    after = r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS), sort=True)
    check_channels(after, twin(r, sc, rows), labels[:448], "after refit_blas")
    assert not same_bits(to_host(after["distance"]), to_host(got["distance"])).all(), "the refit moved nothing these rows see"
    del keep


# ---- 6. the frames around a query ------------------------------------------------------------------------------------------------------
def test_a_query_leaves_frames_and_stats_alone(api):
    sc, rows, labels, want = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    first = r.render()
    r.render_async()
    got = r.query_sweep(dev(rows), tuple(api.QUERY_CHANNELS), sort=True)
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
    """rows written by a torch op, the query, a torch reduction of its answer: one stream, nothing synchronised in between."""
    import torch
    sc, rows, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    reps = 64
    src = dev(rows)
    hit = np.isfinite(want["distance"])
    want_res = (int(hit.sum()) * reps, int(want["triangle_id"].astype(np.int64).sum()) * reps)
    ctx = torch.cuda.stream(torch.cuda.Stream()) if stream == "side" else torch.cuda.stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    with ctx:
        big = torch.empty((len(rows) * reps, 8), dtype=torch.float32, device="cuda")
        big.copy_(src.repeat(reps, 1))                                  # the write the query must wait for
        got = r.query_sweep(big, ("distance", "triangle_id"))
        res = (int(torch.isfinite(got["distance"]).sum()), int(got["triangle_id"].to(torch.int64).sum()))      # the first wait
    assert res == want_res


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
def test_every_error_code_in_order_and_a_valid_query_after_it(api):
    import torch
    sc, rows, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(rows)
    rows_t = dev(rows)
    dist_t = torch.full((n,), -77.0, dtype=torch.float32, device="cuda")
    buf = api.RtxQueryBuffers(); buf.distance = dist_t.data_ptr()
    pp, D, B = rows_t.data_ptr(), api.RTX_QUERY_DISTANCE, C.byref(buf)
    torch.cuda.synchronize()
    cases = [((r.ctx, pp, 0, D, B, 0), INVALID), ((r.ctx, pp, -5, D, B, 0), INVALID), ((r.ctx, None, n, D, B, 0), INVALID), ((r.ctx, pp, n, D, None, 0), INVALID),
             ((r.ctx, pp, n, D | 8, B, 0), INVALID), ((r.ctx, pp, n, 256, B, 0), INVALID), ((r.ctx, pp, n, 0, B, 0), INVALID),
             ((r.ctx, pp, n, D, B, 1), INVALID), ((r.ctx, pp, n, D, B, 16), INVALID), ((r.ctx, pp, n, D, B, 64 | 256), INVALID),      # the ray kernels' flags are not this call's
             ((None, pp, n, D, B, 0), INVALID)]
    for args, code in cases:
        assert lib.rtx_query_sweep(*args) == code, args[2:]
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_sweep(empty.ctx, pp, n, D, B, 0) == STATE
    assert lib.rtx_query_sweep(empty.ctx, pp, n, 0, B, 0) == INVALID              # the argument checks come first
    assert lib.rtx_query_sweep(empty.ctx, pp, n, D, B, 1) == INVALID
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert lib.rtx_query_sweep(rh.ctx, pp, n, D, B, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert lib.rtx_query_sweep(rs.ctx, pp, n, D, B, 0) == LIMIT                   # the stack rule of a render call
    for other in (r, empty, rh, rs):
        other.synchronize()
    assert bool((dist_t == -77).all()), "an error queued something"
    # the walk's own rule, as for rtx_query_nearest: the chain mesh needs (-1 + 1) + (22 + 1) = 23 entries under a TLAS of one leaf, 25 under
    # a TLAS whose deepest inner node is at depth 1
    chain = chain_blas_scene(); chain.config["stack_size"] = 24
    rc = api.Renderer(chain)
    assert lib.rtx_query_sweep(rc.ctx, pp, n, D, B, 0) == 0
    three = copy.deepcopy(chain)
    three.instances = np.concatenate([chain.instances] * 3)
    root = chain.blas[0].nodes[0]
    boxes, centres = [], []
    for k in range(3):
        three.instances["world"][k][3] += 9.0 * k; three.instances["world_inv"][k][3] -= 9.0 * k
        boxes.append(np.concatenate([root["aabb_min"] + (9 * k, 0, 0), root["aabb_max"] + (9 * k, 0, 0)])); centres.append((9.0 * k, 0, 0))
    from pyrtx import host
    three.tlas_nodes, three.tlas_indices = host.tlas_build_balanced(np.array(centres, f32), np.array(boxes, f32))
    rt = api.Renderer(three)
    assert lib.rtx_query_sweep(rt.ctx, pp, n, D, B, 0) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    # a frame with a scaled instance: RTX_ERR_STATE after the checks of a render call (a shallow stack stays RTX_ERR_LIMIT) and before the walk's
    # own stack rule (the three chains, enlarged by 2, are no longer RTX_ERR_LIMIT); the argument checks still come first; nothing is queued
    import affineset
    rn = api.Renderer(affineset.with_linear(three, [affineset.LINEAR["uniform2"]]))
    rsn = api.Renderer(affineset.with_linear(shallow, [affineset.LINEAR["uniform2"]]))
    assert lib.rtx_query_sweep(rn.ctx, pp, n, D, B, 0) == STATE and "rigid" in lib.rtx_last_error(rn.ctx).decode()
    assert lib.rtx_query_sweep(rn.ctx, pp, n, 0, B, 0) == INVALID and lib.rtx_query_sweep(rsn.ctx, pp, n, D, B, 0) == LIMIT
    rn.synchronize(); rsn.synchronize()
    for other in (empty, rh, rs, rc, rt):
        other.synchronize()
    r.synchronize()
    assert "stack" in lib.rtx_last_error(rt.ctx).decode()
    check_channels(r.query_sweep(rows_t, tuple(api.QUERY_CHANNELS)), want, labels, "after the errors")
