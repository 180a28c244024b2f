"""rtx_query_overlap on the GPU: boxes in device tensors, the K smallest (object, triangle) overlaps of every row and its count in device
tensors, bit for bit against the host twin (host.query_overlap / host.query_overlapped, the same code of csrc/rtx_overlap_math.h) run on the
arrays read back from the context:
  * the box classes of tests/boxset.py over seven scenes (a deep TLAS, rows with far more than K overlaps, a left-deep chain whose walk reaches
    the spill region — the walk goes left first and pushes the right child, so `chain_blas`, whose deep child is the right one, holds one entry
    and `left_chain`, the same mesh with every pair of children swapped, holds 23), K in {1, 2, 8} and on two of them every K from 1 to 8, with
    and without a count, count-only, the objects form, query_overlapped, sorted rounds with dead rows planted;
  * batch sizes around a wave and a workgroup, one call that crosses a round, RTX_QUERY_GRID in {1, 2, 3}: full lists followed by empty rows,
    the spill chain followed by shallow rows, tiles reversed with dead tiles between them;
  * consistency with query_nearest on the device; guard elements, out= tensors, raw pointers; scalar, per-row and device-table masks;
  * after update_instances, after build_blas and refit_blas; bounces 0 and no lights; frames and rtx_get_stats unchanged; queued between
    other queries and frames without a wait; every error code in the documented order, then a valid call."""
import copy
import ctypes as C

import numpy as np
import pytest

import boxset
import hitset
import util
from test_gpu_query import dev, host as to_host
from test_gpu_rays import chain_blas_scene, many_instances_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
TILE, LDS_STACK = 256, 16
KEYS = ("object_id", "triangle_id", "count")
SCENES = ["cube", "coincident", "materials_aniso", "chain_blas", "left_chain", "many_instances", "quad_stack"]
_CACHE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def left_chain_scene():
    """chain_blas with the two children of every inner node swapped: the rest of the chain is the LEFT child, so a box that reaches along the
    whole chain leaves one leaf on the stack per step."""
    sc = chain_blas_scene()
    nodes = sc.blas[0].nodes.copy()
    for k in range(2, len(nodes) - 1, 2):
        nodes[[k, k + 1]] = nodes[[k + 1, k]]
    sc.blas[0].nodes = nodes
    return sc


def load_scene(name):
    if name not in _CACHE:
        _CACHE[name] = (chain_blas_scene() if name == "chain_blas" else left_chain_scene() if name == "left_chain" else many_instances_scene() if name == "many_instances" else
                        hitset.quad_stack_scene() if name == "quad_stack" else util.load_golden(name)[0])
    return _CACHE[name]


def read_back(r, sc):
    inst, nodes, idx = r.read_frame_state()
    return (inst, nodes, idx, sc.spheres, sc.planes), [r.read_blas(b) for b in range(len(sc.blas))]


def twin(r, sc, boxes, K=8, count=True, objects=False, mask=None, object_masks=None):
    from pyrtx import host
    state, blas = read_back(r, sc)
    out = host.query_overlap(state, boxes, K, count, objects, blas=blas, mask=mask, object_masks=object_masks)
    out.pop("stack_max")
    return out


def generated(name, seed=7):
    """(scene, boxes (about 200, 10), labels, host answers K = 8 with count from the scene's own arrays), once per run."""
    key = ("set", name, seed)
    if key not in _CACHE:
        from pyrtx import host
        sc = load_scene(name)
        boxes, lab = boxset.generate(sc, 14, seed)
        _CACHE[key] = (sc, np.ascontiguousarray(boxes), lab, host.query_overlap(sc, boxes, 8))
    return _CACHE[key]


def check(got, want, labels=None, what=""):
    """Every array of `got` (tensors or arrays) equal to want's, element for element; names the outputs and the box classes that differ."""
    bad = {}
    for name, g in got.items():
        g = to_host(g) if hasattr(g, "cpu") else g
        ok = (g == want[name][:len(g)]).reshape(len(g), -1).all(axis=1)
        if not ok.all():
            rows = np.flatnonzero(~ok)
            bad[name] = (len(rows), rows[:6].tolist(), {} if labels is None else {boxset.CLASSES[c]: int((labels[rows] == c).sum()) for c in np.unique(labels[rows])})
    assert not bad, (what, bad)


# ---- 1. parity with the host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_host_walk(api, name):
    from pyrtx import host
    sc, boxes, labels, want = generated(name)
    assert 150 <= len(boxes) <= 260
    if name == "left_chain":
        assert want["stack_max"] > LDS_STACK, "this scene is here to reach the spill region"
    if name == "quad_stack":
        assert (want["count"] > 8).sum() >= 24
    r = api.Renderer(sc)
    t = dev(boxes)
    got = r.query_overlap(t, 8)
    assert tuple(got) == KEYS and got["object_id"].shape == (len(boxes), 8) and got["triangle_id"].shape == (len(boxes), 8) and got["count"].shape == (len(boxes),)
    check(got, want, labels, name)
    check(got, twin(r, sc, boxes), labels, f"{name}, arrays read back")
    assert (to_host(got["count"]) > 0).sum() > len(boxes) // 3
    check(r.query_overlap(t, 8, sort=True), want, labels, f"{name} sorted")
    for K in range(1, 9) if name in ("quad_stack", "materials_aniso") else (1, 2, 8):      # every K: the sorted insert and the stride p * K + j at odd K too
        for count in (True, False):
            if K == 8 and count:
                continue
            ref = host.query_overlap(sc, boxes, K, count)
            ref.pop("stack_max")
            out = r.query_overlap(t, K, count=count)
            assert tuple(out) == tuple(ref)
            check(out, ref, labels, f"{name} K {K} count {count}")
    only = r.query_overlap(t, 0)
    assert tuple(only) == ("count",)
    check(only, want, labels, f"{name} count only")
    check(r.query_overlap(t, 0, sort=True), want, labels, f"{name} count only, sorted")
    for K in (8, 3, 0):                                                                     # the objects form
        ref = host.query_overlap(sc, boxes, K, objects=True)
        ref.pop("stack_max")
        for sort in (False, True):
            out = r.query_overlap(t, K, objects=True, sort=sort)
            assert tuple(out) == tuple(ref) and "triangle_id" not in out
            check(out, ref, labels, f"{name} objects K {K} sort {sort}")
    anyw = host.query_overlapped(sc, boxes)
    assert np.array_equal(anyw, (want["count"] > 0).astype(np.int32))
    for sort in (False, True):
        a = r.query_overlapped(t, sort=sort)
        assert a.shape == (len(boxes),) and np.array_equal(to_host(a), anyw), (name, sort, np.flatnonzero(to_host(a) != anyw)[:8])


def test_bounces_zero_and_no_lights(api):
    from pyrtx import scene_io as sio
    sc, boxes, labels, want = generated("cube")
    sc = copy.deepcopy(sc)
    sc.config["bounces"] = 0
    sc.point_lights = np.zeros(0, sio.POINT_LIGHT); sc.spot_lights = np.zeros(0, sio.SPOT_LIGHT); sc.dir_lights = np.zeros(0, sio.DIR_LIGHT)
    r = api.Renderer(sc)
    check(r.query_overlap(dev(boxes), 8), want, labels, "bounces 0, no lights")


# ---- 2. batch sizes, rounds, tiles -----------------------------------------------------------------------------------------------------
def long_set(name, n):
    """(scene, n rows, labels, twin K = 8 / objects K = 8 / any): generated sets of seeds 4 apart, concatenated and cut; once per run."""
    key = ("long", name, n)
    if key not in _CACHE:
        from pyrtx import host
        parts, labs, k = [], [], 0
        while sum(len(p) for p in parts) < n:
            sc, b, lab, _ = generated(name, seed=11 + 4 * k)
            parts.append(b); labs.append(lab); k += 1
        rows = np.ascontiguousarray(np.concatenate(parts)[:n]); labs = np.concatenate(labs)[:n]
        _CACHE[key] = (sc, rows, labs, answers(sc, rows))
    return _CACHE[key]


def answers(sc, rows, blas=None):
    from pyrtx import host
    out = {"list": host.query_overlap(sc, rows, 8, blas=blas), "objects": host.query_overlap(sc, rows, 8, objects=True, blas=blas), "any": {"count": host.query_overlapped(sc, rows, blas=blas)}}
    out["stack_max"] = out["list"].pop("stack_max"); out["objects"].pop("stack_max")
    return out


def run_forms(r, t, sort, n=None):
    return {"list": r.query_overlap(t, 8, n=n, sort=sort), "objects": r.query_overlap(t, 8, objects=True, n=n, sort=sort), "any": {"count": r.query_overlapped(t, n=n, sort=sort)},
            "count only": {"count": r.query_overlap(t, 0, n=n, sort=sort)["count"]}}


def compare(got, want, labels, what):
    for form, out in got.items():
        check(out, want["list" if form == "count only" else form], labels, f"{what}, {form}")


def test_batch_sizes_around_a_wave_and_a_workgroup(api):
    sc, rows, labels, want = long_set("materials_aniso", 300)
    r = api.Renderer(sc)
    t = dev(rows)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for sort in (False, True):
            got = run_forms(r, t, sort, n)
            assert all(len(x) == n for out in got.values() for x in out.values())
            compare(got, want, labels, f"n {n} sort {sort}")


def test_one_call_crosses_a_round(api):
    import torch
    sc, rows, labels, want = long_set("cube", 300)
    r = api.Renderer(sc)
    small = dev(rows)
    got = r.query_overlap(small, 1)
    N = api.RTX_QUERY_CHUNK_RAYS + 3
    reps = (N + len(rows) - 1) // len(rows)
    big = small.repeat(reps, 1)[:N].contiguous()
    for sort in (False, True):
        assert torch.equal(r.query_overlap(big, 0, sort=sort)["count"], got["count"].repeat(reps)[:N]), sort
        assert torch.equal(r.query_overlapped(big, sort=sort), (got["count"] > 0).to(torch.int32).repeat(reps)[:N]), sort
    out = r.query_overlap(big, 1)
    assert torch.equal(out["object_id"], got["object_id"].repeat(reps, 1)[:N]) and torch.equal(out["triangle_id"], got["triangle_id"].repeat(reps, 1)[:N])
    assert torch.equal(out["count"], got["count"].repeat(reps)[:N])


def renderer(api, monkeypatch, sc, grid=None):
    """A fresh context: the knob is read once, in rtx_create."""
    if grid is None:
        monkeypatch.delenv("RTX_QUERY_GRID", raising=False)
    else:
        monkeypatch.setenv("RTX_QUERY_GRID", str(grid))
    return api.Renderer(sc)


def heavy_then_light(name):
    """1333 rows (six tiles): the rows with the most overlaps (quad_stack: full lists; left_chain: the deepest stacks) first, then the rest, the
    rows that touch nothing last: a lane's list, stack and count must not carry over to the row it walks in its next tile."""
    sc, rows, labels, want = long_set(name, 1333)
    order = np.argsort(-want["list"]["count"], kind="stable")
    key = ("heavy", name)
    if key not in _CACHE:
        _CACHE[key] = (sc, np.ascontiguousarray(rows[order]), labels[order], answers(sc, rows[order]))
    return _CACHE[key]


@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("name", ["quad_stack", "left_chain"])
def test_later_tiles_carry_nothing_over(api, monkeypatch, name, grid):
    from pyrtx import host
    sc, rows, labels, want = heavy_then_light(name)
    cnt = want["list"]["count"]
    assert (len(rows) + TILE - 1) // TILE >= 6 and (cnt[:TILE] > 0).all() and (cnt[-TILE:] == 0).all()
    if name == "quad_stack":
        assert (cnt[:2 * TILE] > 8).all(), "two tiles of full lists, then shorter and empty ones"
    else:
        assert host.query_overlap(sc, rows[:TILE], 0)["stack_max"] > LDS_STACK and host.query_overlap(sc, rows[-2 * TILE:], 0)["stack_max"] <= LDS_STACK // 2, "the spill region, then rows that stay in LDS"
    r = renderer(api, monkeypatch, sc, grid)
    t = dev(rows)
    state, blas = read_back(r, sc)
    back = answers(state, rows, blas)
    for sort in (False, True):
        got = run_forms(r, t, sort)
        compare(got, want, labels, f"{name} grid {grid} sort {sort}")
        compare(got, back, labels, f"{name} grid {grid} sort {sort}, arrays read back")


@pytest.mark.parametrize("name", ["quad_stack", "left_chain"])
def test_tiles_in_reverse_order_with_dead_tiles_between(api, monkeypatch, name):
    sc, rows, labels, want = heavy_then_light(name)
    tiles = [np.arange(b, min(b + TILE, len(rows))) for b in range(0, len(rows), TILE)][::-1]
    src = []
    for j, tl in enumerate(tiles):                                   # the ragged tile first, padded to a tile with dead rows; a tile of dead rows alone after the second
        src += [tl, np.full(TILE - len(tl), -1)]
        if j == 1:
            src.append(np.full(TILE, -1))
    src = np.concatenate(src)
    live = src >= 0
    perm = np.zeros((len(src), 10), f32); perm[:, 3:6] = 1.0; perm[:, 6 + np.arange(len(src)) % 4] = np.nan      # dead rows: a NaN in the quaternion
    perm[1::3, 6:] = 0.0                                             # ... or a zero quaternion
    perm[live] = rows[src[live]]
    assert len(perm) == 7 * TILE and boxset.is_dead(perm[~live]).all()
    ref = answers(sc, perm)
    for form in ("list", "objects", "any"):
        for k, a in ref[form].items():
            assert np.array_equal(a[live], want[form][k][src[live]]) and (a[~live] == (0 if k == "count" else -1)).all(), (form, k)
    t = dev(perm)
    for grid in (1, None):
        r = renderer(api, monkeypatch, sc, grid)
        for sort in (False, True):
            compare(run_forms(r, t, sort), ref, None, f"{name} permuted, grid {grid} sort {sort}")


# ---- 3. consistency with the merged queries, on the device -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "coincident", "materials_aniso", "quad_stack"])
def test_consistent_with_query_nearest(api, name):
    from pyrtx import host
    sc, boxes, labels, want = generated(name)
    r = api.Renderer(sc)
    live = ~boxset.is_dead(boxes)
    cnt = to_host(r.query_overlap(dev(boxes), 0)["count"])
    # a row that overlaps something has a surface point within its half diagonal of its centre
    pts = np.zeros((len(boxes), 4), f32); pts[:, :3] = np.where(live[:, None], boxes[:, :3], 0.0)
    pts[:, 3] = np.where(live, np.linalg.norm(boxes[:, 3:6].astype(np.float64), axis=1) * (1 + 2.0 ** -20), 1.0).astype(f32)
    pts[:, 3] = np.maximum(pts[:, 3], f32(1e-30))                    # a point box on a surface: a maximum distance of 0 would be a dead row
    near = to_host(r.query_nearest(dev(pts), "distance")["distance"])
    rows = np.flatnonzero(live & (cnt > 0) & (boxes[:, 3:6].max(axis=1) > 0))
    assert len(rows) > len(boxes) // 3 and np.isfinite(near[rows]).all(), (name, rows[~np.isfinite(near[rows])][:8])
    # a point box at a nearest answer's point, inflated by the nearest query's own bound, overlaps that answer's object
    lo, hi = hitset.world_box(sc)
    diag = float(np.linalg.norm(hi - lo))
    probes = np.zeros((len(boxes), 4), f32); probes[:, :3] = np.where(live[:, None], boxes[:, :3], 0.0); probes[:, 3] = np.inf
    ans = {k: to_host(v) for k, v in r.query_nearest(dev(probes), ("distance", "position", "object_id")).items()}
    ok = np.isfinite(ans["distance"]) & (ans["distance"] < 4 * diag)            # a plane far away: the point's own rounding is beyond any useful bound
    assert ok.sum() > len(boxes) // 2
    at = np.zeros((len(boxes), 10), f32); at[:, 9] = 1.0
    at[:, :3] = np.where(ok[:, None], ans["position"], 0.0)
    pmag = np.linalg.norm(at[:, :3].astype(np.float64), axis=1)
    for i in range(len(at)):
        at[i, 3:6] = host.nearest_distance_bound(8.0 * (float(ans["distance"][i]) if ok[i] else 0.0) + 8.0 * diag, 2.0 * (pmag[i] + diag))
    objs = to_host(r.query_overlap(dev(at), 8, objects=True)["object_id"])
    found = (objs == ans["object_id"][:, None]).any(axis=1)
    assert found[ok].all(), (name, np.flatnonzero(ok & ~found)[:8])


# ---- 4. guards, out= and raw pointers --------------------------------------------------------------------------------------------------
def test_outputs_write_nothing_else(api):
    import torch
    from pyrtx import host
    sc, boxes, labels, _ = generated("quad_stack")
    K, n, pad = 3, len(boxes), 16
    want = host.query_overlap(sc, boxes, K)
    want_obj = host.query_overlap(sc, boxes, K, objects=True)
    anyw = host.query_overlapped(sc, boxes)
    r = api.Renderer(sc)
    t = dev(boxes)

    def sentinels():
        return {"object_id": torch.full((n + pad, K), -77, dtype=torch.int32, device="cuda"), "triangle_id": torch.full((n + pad, K), -77, dtype=torch.int32, device="cuda"),
                "count": torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")}

    def raw(buf, names, m=n, sort=False, **kw):
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        r.query_overlap(t.data_ptr(), out={k: buf[k].data_ptr() for k in names}, n=m, sort=sort, **kw)
        r.synchronize()

    for sort in (False, True):
        full = sentinels()
        raw(full, KEYS, sort=sort, max_hits=K)
        check({k: v[:n] for k, v in full.items()}, want, labels, f"raw pointers, sort {sort}")
        assert all(bool((v[n:] == -77).all()) for v in full.values()), "rows past n were written"
    short = sentinels()
    raw(short, KEYS, m=n - 5, max_hits=K)
    for k, v in short.items():
        assert np.array_equal(to_host(v[:n - 5]), want[k][:n - 5]) and bool((v[n - 5:] == -77).all()), k
    ob = sentinels()
    raw(ob, ("object_id", "count"), max_hits=K, objects=True)
    check({k: ob[k][:n] for k in ("object_id", "count")}, want_obj, labels, "objects, raw pointers")
    assert bool((ob["triangle_id"] == -77).all()) and bool((ob["object_id"][n:] == -77).all()) and bool((ob["count"][n:] == -77).all())
    nc = sentinels()
    raw(nc, ("object_id", "triangle_id"), max_hits=K, count=False)
    assert bool((nc["count"] == -77).all()) and np.array_equal(to_host(nc["triangle_id"][:n]), want["triangle_id"])
    co = sentinels()
    raw(co, ("count",), max_hits=0)
    assert bool((co["object_id"] == -77).all()) and bool((co["triangle_id"] == -77).all()) and np.array_equal(to_host(co["count"][:n]), want["count"]) and bool((co["count"][n:] == -77).all())
    # one id array alone, through the C ABI
    for which in (0, 1):
        one = sentinels()
        torch.cuda.synchronize()
        assert r.lib.rtx_query_overlap(r.ctx, t.data_ptr(), n, K, one["object_id"].data_ptr() if which == 0 else None, one["triangle_id"].data_ptr() if which else None, None, 0) == 0
        r.synchronize()
        hit, miss = ("object_id", "triangle_id") if which == 0 else ("triangle_id", "object_id")
        assert np.array_equal(to_host(one[hit][:n]), want[hit]) and bool((one[miss] == -77).all()) and bool((one["count"] == -77).all()) and bool((one[hit][n:] == -77).all())
    av = torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.query_overlapped(t.data_ptr(), out=av.data_ptr(), n=n)
    r.synchronize()
    assert np.array_equal(to_host(av[:n]), anyw) and bool((av[n:] == -77).all())
    # out= tensors are the ones returned
    mine = {"object_id": torch.empty((n, K), dtype=torch.int32, device="cuda"), "count": torch.empty((n,), dtype=torch.int32, device="cuda")}
    got = r.query_overlap(t, K, out=mine)
    assert got["object_id"] is mine["object_id"] and got["count"] is mine["count"] and got["triangle_id"].shape == (n, K)
    check(got, want, labels, "out= tensors")
    flag = torch.empty((n,), dtype=torch.int32, device="cuda")
    assert r.query_overlapped(t, out=flag) is flag and np.array_equal(to_host(flag), anyw)


# ---- 5. sorted rounds with dead rows ---------------------------------------------------------------------------------------------------
def test_sorted_rounds_answer_row_for_row(api):
    sc, rows, labels, _ = long_set("coincident", 400)
    rng = np.random.default_rng(8)
    rows = rows[rng.permutation(len(rows))].copy()
    rows[::6, 9] = np.nan                                             # planted dead rows
    rows[2::11, 0] = np.inf
    rows[5::13, 4] = -1.0
    rows[3::17, 6:] = 0.0
    rows[7::19, 3] = 0.0                                              # alive, with h.x == 0: the sort key files it with the dead rows, the walk answers it
    r = api.Renderer(sc)
    t = dev(rows)
    for K, count in ((8, True), (2, False), (4, True)):
        ref = twin(r, sc, rows, K, count)
        check(r.query_overlap(t, K, count=count), ref, None, f"unsorted K {K}")
        srt = r.query_overlap(t, K, count=count, sort=True)
        check(srt, ref, None, f"sorted K {K}")
    dead = boxset.is_dead(rows)
    assert dead.sum() > 80 and (to_host(srt["count"])[dead] == 0).all() and (to_host(srt["object_id"])[dead] == -1).all()
    flat = (rows[:, 3] == 0) & ~dead
    assert flat.sum() > 10 and (to_host(srt["count"])[flat] > 0).any()


# ---- 6. masks --------------------------------------------------------------------------------------------------------------------------
def test_masks_scalar_per_row_and_a_device_table(api):
    import torch
    from pyrtx import host
    sc, boxes, labels, want = generated("coincident")
    n = len(boxes)
    M = len(sc.instances) + len(sc.spheres) + len(sc.planes)
    r = api.Renderer(sc)
    t = dev(boxes)
    check(r.query_overlap(t, 8, mask=0xFFFFFFFF), want, labels, "all ones, no table")                       # the filtered kernel, nothing hidden
    z = r.query_overlap(t, 8, mask=0)
    assert not to_host(z["count"]).any() and (to_host(z["object_id"]) == -1).all() and not to_host(r.query_overlapped(t, mask=0)).any()
    om = (1 << (np.arange(M) % 4)).astype(np.uint32)
    rm = np.array([(1, 2, 4, 8, 3, 12, 15, 0)[i % 8] for i in range(n)], np.uint32)
    table_t = torch.from_numpy(om.view(np.int32)).cuda()
    r.set_object_masks(table_t)                                                                              # a device tensor: rtx_update_object_masks
    assert np.array_equal(r.read_object_masks(), om)
    rm_t = torch.from_numpy(rm.view(np.int32)).cuda()
    for sort in (False, True):
        for K, objects in ((8, False), (3, False), (8, True), (0, False)):
            ref = host.query_overlap(sc, boxes, K, objects=objects, mask=rm, object_masks=om); ref.pop("stack_max")
            check(r.query_overlap(t, K, objects=objects, mask=rm_t, sort=sort), ref, labels, f"row masks K {K} objects {objects} sort {sort}")
        assert np.array_equal(to_host(r.query_overlapped(t, mask=rm_t, sort=sort)), host.query_overlapped(sc, boxes, mask=rm, object_masks=om))
        ref = host.query_overlap(sc, boxes, 8, mask=5, object_masks=om); ref.pop("stack_max")
        check(r.query_overlap(t, 8, mask=5, sort=sort), ref, labels, f"scalar mask, sort {sort}")
    got = to_host(r.query_overlap(t, 8, mask=rm_t)["object_id"])
    for i in range(n):
        ids = got[i][got[i] >= 0]
        assert ((om[ids] & rm[i]) != 0).all(), i
    check(r.query_overlap(t, 8), want, labels, "the unfiltered call ignores the table")
    r.set_object_masks(None)
    check(r.query_overlap(t, 8, mask=rm_t), {k: np.where((rm != 0).reshape((-1,) + (1,) * (want[k].ndim - 1)), want[k], 0 if k == "count" else -1) for k in KEYS}, labels, "table dropped")


# ---- 7. device-side scene changes ------------------------------------------------------------------------------------------------------
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
    boxes, labels = boxset.generate(moved, 12, seed=42)
    got = r.query_overlap(dev(boxes), 4)
    check(got, twin(r, sc, boxes, 4), labels, "after update_instances")
    check(r.query_overlap(dev(boxes), 4, objects=True, sort=True), twin(r, sc, boxes, 4, objects=True), labels, "after update_instances, objects, sorted")
    old = api.Renderer(sc).query_overlap(dev(boxes), 4)
    assert not np.array_equal(to_host(old["count"]), to_host(got["count"])), "the poses moved nothing these boxes see"
    assert (to_host(got["count"]) > 0).sum() > len(boxes) // 3
    # a box posed like an instance, with the mesh's own root box: it contains that instance, whatever else it touches
    roots = np.stack([np.concatenate([sc.blas[int(b)].nodes[0]["aabb_min"], sc.blas[int(b)].nodes[0]["aabb_max"]]) for b in sc.instances["blas_id"]]).astype(np.float64)
    own = np.zeros((n, 10), f32)
    for k in range(n):
        m = np.asarray(moved.instances[k]["world"], np.float64).reshape(4, 4)
        own[k, :3] = m[:3, :3] @ (0.5 * (roots[k, :3] + roots[k, 3:])) + m[:3, 3]; own[k, 3:6] = 0.5 * (roots[k, 3:] - roots[k, :3]) * 1.01; own[k, 6:] = rot[k]
    ids = to_host(r.query_overlap(dev(own), 8, objects=True)["object_id"])
    assert all(k in ids[k] for k in range(n))


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
    boxes, labels = boxset.generate(state, 12, seed=51)
    boxes = boxes[np.isfinite(boxes).all(axis=1) | (labels == boxset.CLASSES.index("dead"))]      # the generator aims at triangles, pad slots among them
    got = r.query_overlap(dev(boxes), 4)
    check(got, twin(r, sc, boxes, 4), None, "after build_blas")
    assert (to_host(got["count"]) > 0).sum() > len(boxes) // 4
    hot = r.read_blas(0).tri_hot
    pads = np.flatnonzero(np.isnan(hot["position_0"]).any(axis=1) | np.isnan(hot["position_edge_1"]).any(axis=1) | np.isnan(hot["position_edge_2"]).any(axis=1))
    listed = to_host(r.query_overlap(dev(boxes), 8)["triangle_id"])
    assert len(pads) > 0 and not np.isin(listed, pads).any(), "a NaN pad slot overlaps nothing"
    verts = twin_of("padded")[3]
    moved = dev(deform(verts, "wave", seed=21))
    r.refit_blas(0, moved)
    r.update_instances(p, q)
    after = r.query_overlap(dev(boxes), 4, sort=True)
    check(after, twin(r, sc, boxes, 4), None, "after refit_blas")
    assert not np.array_equal(to_host(after["triangle_id"]), to_host(got["triangle_id"])), "the refit moved nothing these boxes see"
    del keep


# ---- 8. the frames and the queries around a call ---------------------------------------------------------------------------------------
def test_a_query_leaves_frames_and_stats_alone(api):
    sc, boxes, labels, want = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    first = r.render()
    r.render_async()
    got = r.query_overlap(dev(boxes), 8, sort=True)
    flags = r.query_overlapped(dev(boxes))
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    after = r.render()
    for out in (first, after):
        assert out["stats"] == ref["stats"] and util.bit_exact(out["rgb"], ref["rgb"]) and np.array_equal(out["packed"], ref["packed"])
    check(got, want, labels)
    assert np.array_equal(to_host(flags), (want["count"] > 0).astype(np.int32))


def test_queued_between_other_queries_and_frames_without_a_wait(api):
    """One stream, nothing synchronised in between: boxes written by a torch op, a frame, a nearest query, the overlap forms, a hits query, a
    frame, then one reduction of everything."""
    import torch
    from pyrtx import host
    sc, boxes, labels, want = generated("materials_aniso")
    ref_frame = api.Renderer(sc).render()
    r = api.Renderer(sc)
    reps = 64
    src = dev(boxes)
    pts = np.ascontiguousarray(np.concatenate([np.nan_to_num(boxes[:, :3], nan=0.0, posinf=0.0, neginf=0.0), np.full((len(boxes), 1), np.inf, f32)], axis=1))
    seg = np.ascontiguousarray(np.concatenate([pts[:, :3], np.tile(f32([0.3, -0.5, 0.8]), (len(boxes), 1)), np.full((len(boxes), 1), 50.0, f32)], axis=1))
    want_near = host.query_nearest(sc, pts, "object_id")["object_id"]
    want_hits = host.query_hits(sc, seg, 0, ())["count"]
    wo = host.query_overlap(sc, boxes, 8, objects=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        big = torch.empty((len(boxes) * reps, 10), dtype=torch.float32, device="cuda")
        big.copy_(src.repeat(reps, 1))                                  # the write the query must wait for
        r.render_async()
        near = r.query_nearest(dev(pts), "object_id")
        a = r.query_overlap(big, 2)
        b = r.query_overlapped(big, sort=True)
        c = r.query_overlap(big, 8, objects=True)
        hits = r.query_hits(dev(seg), 0, ())
        d = r.query_overlap(big, 0, sort=True)
        r.render_async()
        res = (int(a["count"].to(torch.int64).sum()), int(a["triangle_id"].to(torch.int64).sum()), int(b.to(torch.int64).sum()), int(c["object_id"].to(torch.int64).sum()),
               int(d["count"].to(torch.int64).sum()))                   # the first wait
        near_h, hits_h = to_host(near["object_id"]), to_host(hits["count"])
    total = int(want["count"].astype(np.int64).sum())
    assert res == (total * reps, int(want["triangle_id"][:, :2].astype(np.int64).sum()) * reps, int((want["count"] > 0).sum()) * reps, int(wo["object_id"].astype(np.int64).sum()) * reps, total * reps)
    assert np.array_equal(near_h, want_near) and np.array_equal(hits_h, want_hits)
    r.synchronize()
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref_frame["stats"] and util.bit_exact(rgb, ref_frame["rgb"]) and np.array_equal(packed, ref_frame["packed"])


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------------
def test_every_error_code_in_order_and_a_valid_query_after_it(api):
    import torch
    from pyrtx import host
    sc, boxes, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(boxes)
    t = dev(boxes)
    obj_t = torch.full((n, 2), -77, dtype=torch.int32, device="cuda"); tri_t = torch.full((n, 2), -77, dtype=torch.int32, device="cuda")
    cnt_t = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    pp, op, tp, cp = t.data_ptr(), obj_t.data_ptr(), tri_t.data_ptr(), cnt_t.data_ptr()
    OBJ, ANY, SORT = api.RTX_OVERLAP_OBJECTS, api.RTX_OVERLAP_ANY, api.RTX_QUERY_SORT
    torch.cuda.synchronize()
    # (ctx, boxes, n, max_hits, object_id, triangle_id, count, flags)
    cases = [(r.ctx, pp, n, 9, op, tp, cp, 0), (r.ctx, pp, n, -1, op, tp, cp, 0),                                        # max_hits
             (r.ctx, pp, n, 2, op, None, cp, ANY), (r.ctx, pp, n, 0, None, None, cp, ANY | OBJ),                          # ANY needs max_hits == 0 and excludes OBJECTS
             (r.ctx, pp, n, 2, op, tp, cp, OBJ),                                                                          # OBJECTS forbids triangle ids
             (r.ctx, pp, n, 0, None, None, None, 0), (r.ctx, pp, n, 0, op, tp, None, 0), (r.ctx, pp, n, 0, None, None, None, ANY),      # max_hits == 0 needs a count
             (r.ctx, pp, n, 2, None, None, cp, 0), (r.ctx, pp, n, 2, None, None, cp, OBJ),                                # max_hits > 0 needs an id array
             (r.ctx, None, n, 2, op, tp, cp, 0), (r.ctx, pp, 0, 2, op, tp, cp, 0), (r.ctx, pp, -5, 2, op, tp, cp, 0),     # the rows
             (r.ctx, pp, n, 2, op, tp, cp, 1), (r.ctx, pp, n, 2, op, tp, cp, 16), (r.ctx, pp, n, 2, op, tp, cp, 64 | SORT), (r.ctx, pp, n, 2, op, tp, cp, 2048),      # flags
             (None, pp, n, 2, op, tp, cp, 0)]
    for args in cases:
        assert lib.rtx_query_overlap(*args) == INVALID, args[2:]
    filt = api.RtxQueryFilter(None, 1)
    assert lib.rtx_query_overlap_filtered(r.ctx, pp, n, 9, op, tp, cp, 0, C.byref(filt)) == INVALID
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_overlap(empty.ctx, pp, n, 2, op, tp, cp, 0) == STATE
    assert lib.rtx_query_overlap(empty.ctx, pp, n, 0, None, None, cp, ANY) == STATE
    assert lib.rtx_query_overlap(empty.ctx, pp, n, 2, op, tp, cp, OBJ) == INVALID          # the argument checks come first
    assert lib.rtx_query_overlap(empty.ctx, pp, n, 2, op, tp, cp, 1) == INVALID
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert lib.rtx_query_overlap(rh.ctx, pp, n, 2, op, tp, cp, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert lib.rtx_query_overlap(rs.ctx, pp, n, 2, op, tp, cp, 0) == LIMIT                 # the stack rule of a render call
    # the walk's own rule, that of rtx_query_nearest: the chain mesh needs (-1 + 1) + (22 + 1) = 23 entries under a TLAS of one leaf, 25 under
    # a TLAS whose deepest inner node is at depth 1
    chain = chain_blas_scene(); chain.config["stack_size"] = 24
    rc = api.Renderer(chain)
    assert lib.rtx_query_overlap(rc.ctx, pp, n, 2, op, tp, cp, 0) == 0
    three = copy.deepcopy(chain)
    three.instances = np.concatenate([chain.instances] * 3)
    root = chain.blas[0].nodes[0]
    bxs, centres = [], []
    for k in range(3):
        three.instances["world"][k][3] += 9.0 * k; three.instances["world_inv"][k][3] -= 9.0 * k
        bxs.append(np.concatenate([root["aabb_min"] + (9 * k, 0, 0), root["aabb_max"] + (9 * k, 0, 0)])); centres.append((9.0 * k, 0, 0))
    three.tlas_nodes, three.tlas_indices = host.tlas_build_balanced(np.array(centres, f32), np.array(bxs, f32))
    rt = api.Renderer(three)
    assert lib.rtx_query_overlap(rt.ctx, pp, n, 2, op, tp, cp, 0) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    assert lib.rtx_query_overlap(rt.ctx, pp, n, 0, None, None, cp, ANY) == LIMIT
    # a frame with a scaled instance: RTX_ERR_STATE after the checks of a render call (a shallow stack stays RTX_ERR_LIMIT) and before the walk's
    # own stack rule (the three chains, enlarged by 2, are no longer RTX_ERR_LIMIT); the argument checks still come first; nothing is queued
    import affineset
    rn = api.Renderer(affineset.with_linear(three, [affineset.LINEAR["uniform2"]]))
    rsn = api.Renderer(affineset.with_linear(shallow, [affineset.LINEAR["uniform2"]]))
    assert lib.rtx_query_overlap(rn.ctx, pp, n, 2, op, tp, cp, 0) == STATE and "rigid" in lib.rtx_last_error(rn.ctx).decode()
    assert lib.rtx_query_overlap(rn.ctx, pp, n, 0, None, None, cp, ANY) == STATE and lib.rtx_query_overlap_filtered(rn.ctx, pp, n, 2, op, tp, cp, 0, C.byref(filt)) == STATE
    assert lib.rtx_query_overlap(rn.ctx, pp, n, 9, op, tp, cp, 0) == INVALID and lib.rtx_query_overlap(rsn.ctx, pp, n, 2, op, tp, cp, 0) == LIMIT
    rn.synchronize(); rsn.synchronize()
    assert "stack" in lib.rtx_last_error(rt.ctx).decode()
    # the state rule of the filtered call comes last: a table set for other counts than the frame's
    r.set_object_masks(np.full(len(sc.instances) + len(sc.spheres) + len(sc.planes), 1, np.uint32))
    fewer = copy.deepcopy(sc); fewer.spheres = fewer.spheres[:-1]
    r.set_frame(fewer)
    assert lib.rtx_query_overlap_filtered(r.ctx, pp, n, 2, op, tp, cp, 0, C.byref(filt)) == STATE
    assert lib.rtx_query_overlap_filtered(r.ctx, pp, n, 2, op, tp, cp, 2048, C.byref(filt)) == INVALID
    assert lib.rtx_query_overlap(r.ctx, pp, n, 2, op, tp, cp, 0) == 0                       # the unfiltered call does not look at the table
    r.set_frame(sc)
    r.set_object_masks(None)
    for other in (empty, rh, rs, rc, rt):
        other.synchronize()
    r.synchronize()
    obj_t.fill_(-77); tri_t.fill_(-77); cnt_t.fill_(-77)
    torch.cuda.synchronize()
    for args in cases[:-1]:                                                   # an error queues nothing
        lib.rtx_query_overlap(*args)
    r.synchronize()
    assert bool((obj_t == -77).all()) and bool((tri_t == -77).all()) and bool((cnt_t == -77).all())
    check(r.query_overlap(t, 8), want, labels, "after the errors")
