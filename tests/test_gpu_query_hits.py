"""rtx_query_hits on the GPU: segments in device tensors, the first K hits of every row and its count in device tensors, every channel bit for
bit (NaN == NaN) against the host twin (host.query_hits, the same code of csrc/rtx_hits_math.h) run on the arrays read back from the context:
  * the segment classes of tests/hitset.py over seven scenes (a stack past RTX_LDS_STACK, a deep TLAS, rows with more than K hits), K in
    {1, 2, 8} and on two of them every K from 1 to 8, with and without a count, the count-only form, sorted rounds;
  * batch sizes around a wave and a workgroup, one call that crosses a round;
  * consistency with the merged queries on the device: query_closest's hit is in the list and never nearer than its head, the head's channels
    are query_closest's, query_occluded is count > 0 where the scene has no sphere;
  * channel subsets and guard elements with K = 3, out= tensors, raw pointers; sort=True with dead rows planted;
  * after update_instances, after build_blas and refit_blas; bounces 0 and no lights; frames and rtx_get_stats unchanged; stream order;
  * every error code in the documented order, then a valid call."""
import copy
import ctypes as C

import numpy as np
import pytest

import hitset
import util
from test_gpu_query import dev, host as to_host, same_bits
from test_gpu_rays import chain_blas_scene, many_instances_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
ALL = hitset.ALL
SCENES = ["cube", "coincident", "materials_aniso", "chain_blas", "many_instances", "quad_stack", "slab_chain"]
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
    if name == "quad_stack":
        return hitset.quad_stack_scene()
    if name == "slab_chain":
        return hitset.slab_chain_scene()
    return util.load_golden(name)[0]


def read_back(r, sc):
    """What the context holds, as host.query_hits takes it."""
    inst, nodes, idx = r.read_frame_state()
    return (inst, nodes, idx, sc.spheres, sc.planes), [r.read_blas(b) for b in range(len(sc.blas))]


def twin(r, sc, seg, K, channels=ALL, count=True):
    from pyrtx import host
    state, blas = read_back(r, sc)
    out = host.query_hits(state, seg, K, channels, count, blas=blas)
    out.pop("stack_max")
    return out


def generated(name, seed=5):
    """(scene, segments (about 210, 7), labels, host answers K = 8 with count from the scene's own arrays), once per run."""
    key = (name, seed)
    if key not in _CACHE:
        from pyrtx import host
        from test_query_hits_cpu import stack_rays
        sc = load_scene(name)
        seg, lab = hitset.generate(sc, 18, seed)
        if name in ("quad_stack", "slab_chain"):
            extra = stack_rays(sc, 24, 6) if name == "quad_stack" else hitset.chain_rays(8)
            seg = np.concatenate([seg, extra]); lab = np.concatenate([lab, np.full(len(extra), hitset.CLASSES.index("through"))])
        _CACHE[key] = (sc, np.ascontiguousarray(seg), lab, host.query_hits(sc, seg, 8, ALL))
    return _CACHE[key]


def check(got, want, labels=None, what=""):
    """Every array of `got` (tensors or arrays, the count included) bit for bit; names the channels and the segment classes that differ."""
    bad = {}
    for name, g in got.items():
        g = to_host(g) if hasattr(g, "cpu") else g
        ok = same_bits(g, want[name][:len(g)])
        if not ok.all():
            rows = np.flatnonzero(~ok)
            bad[name] = (len(rows), rows[:6].tolist(), {} if labels is None else {hitset.CLASSES[c]: int((labels[rows] == c).sum()) for c in np.unique(labels[rows])})
    assert not bad, (what, bad)


# ---- 1. parity with the host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_host_walk(api, name):
    from pyrtx import host
    sc, seg, labels, want = generated(name)
    assert 150 <= len(seg) <= 260
    if name == "slab_chain":
        assert want["stack_max"] > 16, "this scene is here to reach the spill region"          # RTX_LDS_STACK
    if name == "quad_stack":
        assert (want["count"] > 8).sum() >= 12
    r = api.Renderer(sc)
    seg_t = dev(seg)
    got = r.query_hits(seg_t, 8, ALL)
    assert tuple(got) == ALL + ("count",) and got["distance"].shape == (len(seg), 8) and got["position"].shape == (len(seg), 8, 3) and got["uv"].shape == (len(seg), 8, 2)
    check(got, want, labels, name)
    check(got, twin(r, sc, seg, 8), labels, f"{name}, arrays read back")
    assert (to_host(got["count"]) > 0).sum() > len(seg) // 3
    check(r.query_hits(seg_t, 8, ALL, sort=True), want, labels, f"{name} sorted")
    for K in range(1, 9) if name in ("quad_stack", "materials_aniso") else (1, 2, 8):      # every K: the sorted insert, the K-th-hit bound and the stride p * K + j at odd K too
        for count in (True, False):
            if K == 8 and count:
                continue
            ref = host.query_hits(sc, seg, K, ALL, count)
            ref.pop("stack_max")
            out = r.query_hits(seg_t, K, ALL, count=count)
            assert tuple(out) == tuple(ref)
            check(out, ref, labels, f"{name} K {K} count {count}")
    only = r.query_hits(seg_t, 0, ())
    assert tuple(only) == ("count",)
    check(only, want, labels, f"{name} count only")
    check(r.query_hits(seg_t, 0, (), sort=True), want, labels, f"{name} count only, sorted")


def test_bounces_zero_and_no_lights(api):
    from pyrtx import scene_io as sio
    sc, seg, labels, want = generated("cube")
    sc = copy.deepcopy(sc)
    sc.config["bounces"] = 0
    sc.point_lights = np.zeros(0, sio.POINT_LIGHT); sc.spot_lights = np.zeros(0, sio.SPOT_LIGHT); sc.dir_lights = np.zeros(0, sio.DIR_LIGHT)
    r = api.Renderer(sc)
    check(r.query_hits(dev(seg), 8, ALL), want, labels, "bounces 0, no lights")


# ---- 2. batch sizes and rounds ---------------------------------------------------------------------------------------------------------
def two_sets(name):
    sc, a, la, _ = generated(name)
    _, b, lb, _ = generated(name, seed=9)
    return sc, np.ascontiguousarray(np.concatenate([a, b]))


def test_batch_sizes_around_a_wave_and_a_workgroup(api):
    from pyrtx import host
    sc, seg = two_sets("materials_aniso")
    assert len(seg) >= 257
    want = host.query_hits(sc, seg, 1, "distance")
    r = api.Renderer(sc)
    seg_t = dev(seg)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for sort in (False, True):
            only = r.query_hits(seg_t, 0, (), n=n, sort=sort)
            one = r.query_hits(seg_t, 1, "distance", n=n, sort=sort)
            assert only["count"].shape == (n,) and one["distance"].shape == (n, 1) and one["count"].shape == (n,)
            check(only, want, None, f"count only, n {n} sort {sort}")
            check(one, want, None, f"K 1, n {n} sort {sort}")


def test_one_call_crosses_a_round(api):
    import torch
    sc, seg = two_sets("materials_aniso")
    r = api.Renderer(sc)
    small = dev(seg)
    got = r.query_hits(small, 1, "distance")
    N = api.RTX_QUERY_CHUNK_RAYS + 3
    reps = (N + len(seg) - 1) // len(seg)
    big = small.repeat(reps, 1)[:N].contiguous()
    for sort in (False, True):
        only = r.query_hits(big, 0, (), sort=sort)
        assert torch.equal(only["count"], got["count"].repeat(reps)[:N]), sort
    out = r.query_hits(big, 1, "distance")
    assert torch.equal(out["distance"].view(torch.int32), got["distance"].view(torch.int32).repeat(reps, 1)[:N])
    assert torch.equal(out["count"], got["count"].repeat(reps)[:N])


# ---- 3. consistency with the merged queries, on the device -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_consistent_with_query_closest_and_query_occluded(api, name):
    sc, seg, labels, _ = generated(name)
    r = api.Renderer(sc)
    K = 8
    far = seg.copy(); far[:, 6] = np.inf
    hits = {k: to_host(t) for k, t in r.query_hits(dev(far), K, ALL).items()}
    closest = {k: to_host(t) for k, t in r.query_closest(dev(np.ascontiguousarray(far[:, :6])), ALL).items()}
    cd = closest["distance"]
    assert not np.isnan(cd).any() and (hits["distance"][:, 0] <= cd).all(), np.flatnonzero(~(hits["distance"][:, 0] <= cd))[:8]      # a miss is +inf on both sides
    is_closest = ((hits["distance"].view(np.uint32) == cd.view(np.uint32)[:, None]) & (hits["object_id"] == closest["object_id"][:, None])
                  & (hits["triangle_id"] == closest["triangle_id"][:, None]))
    rows = np.flatnonzero((hits["count"] <= K) & np.isfinite(cd))
    assert len(rows) > len(seg) // 4
    assert is_closest[rows].any(axis=1).all(), (name, rows[~is_closest[rows].any(axis=1)][:8])
    # where the closest hit is the head of the list, every channel is query_closest's: the accept branches restated are the production ones
    head = np.flatnonzero(np.isfinite(cd) & is_closest[:, 0])
    assert len(head) > len(seg) // 4
    for ch in ALL:
        assert same_bits(hits[ch][head, 0], closest[ch][head]).all(), (name, ch, head[~same_bits(hits[ch][head, 0], closest[ch][head])][:8])
    if len(sc.spheres) == 0:                                                 # Sphere::intersect is other arithmetic than Sphere::trace
        count = to_host(r.query_hits(dev(seg), 0, ())["count"])
        occ = to_host(r.query_occluded(dev(seg)))
        assert np.array_equal(occ != 0, count > 0), (name, np.flatnonzero((occ != 0) != (count > 0))[:8])
        assert 10 < (count > 0).sum() < len(seg) - 10


def test_scenes_without_spheres_are_checked_against_query_occluded():
    assert sum(len(load_scene(n).spheres) == 0 for n in SCENES) >= 3


# ---- 4. channel subsets, guards, out= and raw pointers ---------------------------------------------------------------------------------
def test_channel_subsets_write_nothing_else(api):
    import torch
    from pyrtx import host
    sc, seg, labels, _ = generated("quad_stack")
    K, n, pad = 3, len(seg), 16
    want = host.query_hits(sc, seg, K, ALL)
    r = api.Renderer(sc)
    seg_t = dev(seg)

    def sentinels():
        out = {}
        for name, (_, dt, k) in api.QUERY_CHANNELS.items():
            shape = (n + pad, K, k) if k > 1 else (n + pad, K)
            out[name] = torch.full(shape, -77.0, dtype=torch.float32, device="cuda") if dt == np.float32 else torch.full(shape, -77, dtype=torch.int32, device="cuda")
        out["count"] = torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")
        return out

    def run(names, buffers, count=True, sort=False, m=n):
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        r.query_hits(seg_t.data_ptr(), K, names, count, out={k: buffers[k].data_ptr() for k in tuple(names) + (("count",) if count else ())}, n=m, sort=sort)
        r.synchronize()

    for sort in (False, True):
        full = sentinels()
        run(ALL, full, sort=sort)
        check({k: t[:n] for k, t in full.items()}, want, labels, f"all channels, raw pointers, sort {sort}")
        for k, t in full.items():
            assert bool((t[n:] == -77).all()), f"{k}: rows past n were written"
    short = sentinels()                                                     # n - 5 rows: the entries of the other rows are untouched
    run(ALL, short, m=n - 5)
    for k, t in short.items():
        assert same_bits(to_host(t[:n - 5]), want[k][:n - 5]).all() and bool((t[n - 5:] == -77).all()), k
    for names in (("distance",), ("position",), ("normal", "uv"), ("material_id",), ("object_id", "triangle_id")):
        for count in (True, False):
            part = sentinels()
            run(names, part, count)
            ref = want if count else host.query_hits(sc, seg, K, ALL, count=False)
            for k, t in part.items():
                if k in names or (k == "count" and count):
                    assert same_bits(to_host(t[:n]), ref[k]).all() and bool((t[n:] == -77).all()), (names, count, k)
                else:
                    assert bool((t == -77).all()), f"{k} was not requested with {names}, count {count}"
    # a bit without a pointer, and a pointer without its bit: neither is written
    both = sentinels()
    buf = api.RtxQueryBuffers()
    buf.distance = both["distance"].data_ptr(); buf.normal = both["normal"].data_ptr()
    torch.cuda.synchronize()
    assert r.lib.rtx_query_hits(r.ctx, seg_t.data_ptr(), n, K, api.RTX_QUERY_DISTANCE | api.RTX_QUERY_UV, C.byref(buf), None, 0) == 0
    r.synchronize()
    assert same_bits(to_host(both["distance"][:n]), host.query_hits(sc, seg, K, "distance", count=False)["distance"]).all()
    assert bool((both["normal"] == -77).all()) and bool((both["uv"] == -77).all()) and bool((both["count"] == -77).all())
    # out= tensors are the ones returned
    mine = {"distance": torch.empty((n, K), dtype=torch.float32, device="cuda"), "normal": torch.empty((n, K, 3), dtype=torch.float32, device="cuda"),
            "count": torch.empty((n,), dtype=torch.int32, device="cuda")}
    got = r.query_hits(seg_t, K, ("distance", "normal", "object_id"), out=mine)
    assert got["distance"] is mine["distance"] and got["normal"] is mine["normal"] and got["count"] is mine["count"] and got["object_id"].shape == (n, K)
    check(got, want, labels, "out= tensors")


# ---- 5. sorted rounds ------------------------------------------------------------------------------------------------------------------
def test_sorted_rounds_answer_row_for_row(api):
    sc, seg = two_sets("coincident")
    rng = np.random.default_rng(8)
    seg = seg[rng.permutation(len(seg))].copy()
    seg[::6, 6] = rng.choice(np.array([0.0, -2.0, np.nan], f32), size=len(seg[::6]))          # planted dead rows
    seg[2::11, 0] = np.nan
    seg[5::13, 3:6] = 0.0
    r = api.Renderer(sc)
    t = dev(seg)
    for K, count in ((8, True), (2, False), (4, True)):
        plain = r.query_hits(t, K, ALL, count=count)
        srt = r.query_hits(t, K, ALL, count=count, sort=True)
        ref = twin(r, sc, seg, K, ALL, count)
        check(plain, ref, None, f"unsorted K {K}")
        check(srt, ref, None, f"sorted K {K}")
    dead = hitset.is_dead(seg)
    assert dead.sum() > 40 and (to_host(srt["count"])[dead] == 0).all() and np.isinf(to_host(srt["distance"])[dead]).all() and (to_host(srt["object_id"])[dead] == -1).all()


# ---- 6. device-side scene changes ------------------------------------------------------------------------------------------------------
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
    seg, labels = hitset.generate(moved, 16, seed=42)
    got = r.query_hits(dev(seg), 4, ALL)
    check(got, twin(r, sc, seg, 4), labels, "after update_instances")
    check(r.query_hits(dev(seg), 4, ALL, count=False, sort=True), twin(r, sc, seg, 4, ALL, False), labels, "after update_instances, sorted, no count")
    old = api.Renderer(sc).query_hits(dev(seg), 4, ("distance",))
    assert not same_bits(to_host(old["count"]), to_host(got["count"])).all(), "the poses moved nothing these segments see"
    assert (to_host(got["count"]) > 0).sum() > len(seg) // 3


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
    seg, labels = hitset.generate(state, 14, seed=51)
    seg = seg[np.isfinite(seg[:, :6]).all(axis=1) | (labels == hitset.CLASSES.index("dead"))]      # the generator aims at triangles, pad slots among them
    got = r.query_hits(dev(seg), 4, ALL)
    check(got, twin(r, sc, seg, 4), None, "after build_blas")
    assert (to_host(got["count"]) > 0).sum() > len(seg) // 4
    verts = twin_of("padded")[3]
    moved = dev(deform(verts, "wave", seed=21))
    r.refit_blas(0, moved)
    r.update_instances(p, q)
    after = r.query_hits(dev(seg), 4, ALL, sort=True)
    check(after, twin(r, sc, seg, 4), None, "after refit_blas")
    assert not same_bits(to_host(after["distance"]), to_host(got["distance"])).all(), "the refit moved nothing these segments see"
    del keep


# ---- 7. the frames around a query ------------------------------------------------------------------------------------------------------
def test_a_query_leaves_frames_and_stats_alone(api):
    sc, seg, labels, want = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    first = r.render()
    r.render_async()
    got = r.query_hits(dev(seg), 8, ALL, sort=True)
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    after = r.render()
    for out in (first, after):
        assert out["stats"] == ref["stats"] and util.bit_exact(out["rgb"], ref["rgb"]) and np.array_equal(out["packed"], ref["packed"])
    check(got, want, labels)


# ---- 8. stream order -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["side", "default"])
def test_queries_are_ordered_on_torchs_stream(api, stream):
    """segments written by a torch op, the query, a torch reduction of its answer: one stream, nothing synchronised in between."""
    import torch
    sc, seg, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    reps = 256
    src = dev(seg)
    want_res = (int(want["count"].astype(np.int64).sum()) * reps, int(want["triangle_id"][:, :2].astype(np.int64).sum()) * reps)
    ctx = torch.cuda.stream(torch.cuda.Stream()) if stream == "side" else torch.cuda.stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    with ctx:
        big = torch.empty((len(seg) * reps, 7), dtype=torch.float32, device="cuda")
        big.copy_(src.repeat(reps, 1))                                  # the write the query must wait for
        got = r.query_hits(big, 2, ("triangle_id",))
        res = (int(got["count"].to(torch.int64).sum()), int(got["triangle_id"].to(torch.int64).sum()))      # the first wait
    assert res == want_res


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------------
def test_every_error_code_in_order_and_a_valid_query_after_it(api):
    import torch
    sc, seg, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(seg)
    seg_t = dev(seg)
    dist_t = torch.full((n, 2), -77.0, dtype=torch.float32, device="cuda")
    cnt_t = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    buf = api.RtxQueryBuffers(); buf.distance = dist_t.data_ptr()
    pp, D, B, cp = seg_t.data_ptr(), api.RTX_QUERY_DISTANCE, C.byref(buf), cnt_t.data_ptr()
    torch.cuda.synchronize()
    # (ctx, segments, n, max_hits, channels, out, count, flags)
    cases = [(r.ctx, pp, 0, 2, D, B, cp, 0), (r.ctx, pp, -5, 2, D, B, cp, 0), (r.ctx, None, n, 2, D, B, cp, 0), (r.ctx, pp, n, 2, D, None, cp, 0),
             (r.ctx, pp, n, 2, D | 8, B, cp, 0), (r.ctx, pp, n, 2, 256, B, cp, 0), (r.ctx, pp, n, 2, 0, B, cp, 0),                  # channels
             (r.ctx, pp, n, 9, D, B, cp, 0), (r.ctx, pp, n, -1, D, B, cp, 0), (r.ctx, pp, n, 0, D, B, cp, 0), (r.ctx, pp, n, 0, 0, B, None, 0),   # max_hits / the count-only form
             (r.ctx, pp, n, 2, D, B, cp, 1), (r.ctx, pp, n, 2, D, B, cp, 16), (r.ctx, pp, n, 2, D, B, cp, 64 | 256),             # the ray kernels' flags are not this call's
             (None, pp, n, 2, D, B, cp, 0)]
    for args in cases:
        assert lib.rtx_query_hits(*args) == INVALID, args[2:]
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_hits(empty.ctx, pp, n, 2, D, B, cp, 0) == STATE
    assert lib.rtx_query_hits(empty.ctx, pp, n, 0, 0, None, cp, 0) == STATE
    assert lib.rtx_query_hits(empty.ctx, pp, n, 2, 0, B, cp, 0) == INVALID            # the argument checks come first
    assert lib.rtx_query_hits(empty.ctx, pp, n, 2, D, B, cp, 1) == INVALID
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert lib.rtx_query_hits(rh.ctx, pp, n, 2, D, B, cp, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert lib.rtx_query_hits(rs.ctx, pp, n, 2, D, B, cp, 0) == LIMIT                 # the stack rule of a render call
    # the walk's own rule, that of rtx_query_nearest: the chain mesh needs (-1 + 1) + (22 + 1) = 23 entries under a TLAS of one leaf, 25 under
    # a TLAS whose deepest inner node is at depth 1
    chain = chain_blas_scene(); chain.config["stack_size"] = 24
    rc = api.Renderer(chain)
    assert lib.rtx_query_hits(rc.ctx, pp, n, 2, D, B, cp, 0) == 0
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
    assert lib.rtx_query_hits(rt.ctx, pp, n, 2, D, B, cp, 0) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    assert lib.rtx_query_hits(rt.ctx, pp, n, 0, 0, None, cp, 0) == LIMIT
    for other in (empty, rh, rs, rc, rt):
        other.synchronize()
    r.synchronize()
    assert "stack" in lib.rtx_last_error(rt.ctx).decode()
    dist_t.fill_(-77.0); cnt_t.fill_(-77)
    torch.cuda.synchronize()
    for args in cases[:-1]:                                                   # an error queues nothing
        lib.rtx_query_hits(*args)
    r.synchronize()
    assert bool((dist_t == -77).all()) and bool((cnt_t == -77).all())
    check(r.query_hits(seg_t, 8, ALL), want, labels, "after the errors")
