"""rtx_query_overlap_capsule on the GPU: capsules in device tensors, the K smallest (object, triangle) overlaps of every row and its count
in device tensors, bit for bit against the host twin (host.query_overlap_capsule / host.query_overlapped_capsule, the same code of
csrc/rtx_capsule_math.h) run on the arrays read back from the context:
  * the classes of tests/capsuleset.py over eight scenes (a deep TLAS, rows with far more than K overlaps, a chain of slabs, a left-deep
    chain whose walk reaches the spill region, a golden scene with spheres and planes), every form, K in {1, 4, 8} and count-only, sorted
    rounds with dead and ball rows mixed in;
  * batch sizes around a wave and a workgroup, one call that crosses a round, RTX_QUERY_GRID in {1, 2}: full lists followed by empty rows;
  * two cross-checks on the device: a ball row against query_nearest, a capsule against query_sweep along its axis;
  * guard elements, out= tensors, raw pointers; scalar, per-row and device-table masks; the identity forms against the unfiltered call;
  * after update_instances, after build_blas and refit_blas; frames and rtx_get_stats unchanged; every error code in the documented order,
    a non-rigid frame refused and accepted again after update_instances."""
import copy
import ctypes as C

import numpy as np
import pytest

import capsuleset
import hitset
import util
from test_gpu_query import dev, host as to_host
from test_gpu_query_overlap import left_chain_scene, read_back, renderer
from test_gpu_rays import chain_blas_scene, many_instances_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
TILE, LDS_STACK = 256, 16
KEYS = ("object_id", "triangle_id", "count")
SCENES = ["cube", "coincident", "materials_aniso", "chain_blas", "left_chain", "many_instances", "quad_stack", "slab_chain"]
_CACHE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def load_scene(name):
    if name not in _CACHE:
        _CACHE[name] = (chain_blas_scene() if name == "chain_blas" else left_chain_scene() if name == "left_chain" else many_instances_scene() if name == "many_instances" else
                        hitset.quad_stack_scene() if name == "quad_stack" else hitset.slab_chain_scene() if name == "slab_chain" else util.load_golden(name)[0])
    return _CACHE[name]


def twin(r, sc, rows, K=8, count=True, objects=False, mask=None, object_masks=None):
    from pyrtx import host
    state, blas = read_back(r, sc)
    out = host.query_overlap_capsule(state, rows, K, count, objects, blas=blas, mask=mask, object_masks=object_masks)
    out.pop("stack_max")
    return out


def generated(name, seed=7):
    """(scene, rows (about 150, 7), labels, host answers K = 8 with count from the scene's own arrays), once per run."""
    key = ("set", name, seed)
    if key not in _CACHE:
        from pyrtx import host
        sc = load_scene(name)
        rows, lab = capsuleset.generate(sc, 9, seed)
        _CACHE[key] = (sc, np.ascontiguousarray(rows), lab, host.query_overlap_capsule(sc, rows, 8))
    return _CACHE[key]


def check(got, want, labels=None, what=""):
    """Every array of `got` (tensors or arrays) equal to want's, element for element; names the outputs and the classes that differ."""
    bad = {}
    for name, g in got.items():
        g = to_host(g) if hasattr(g, "cpu") else g
        ok = (g == want[name][:len(g)]).reshape(len(g), -1).all(axis=1)
        if not ok.all():
            rows = np.flatnonzero(~ok)
            bad[name] = (len(rows), rows[:6].tolist(), {} if labels is None else {capsuleset.CLASSES[c]: int((labels[rows] == c).sum()) for c in np.unique(labels[rows])})
    assert not bad, (what, bad)


# ---- 1. parity with the host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_host_walk(api, name):
    from pyrtx import host
    sc, rows, labels, want = generated(name)
    assert 120 <= len(rows) <= 200
    if name == "left_chain":
        assert want["stack_max"] > LDS_STACK, "this scene is here to reach the spill region"
    if name == "quad_stack":
        assert (want["count"] > 8).sum() >= 12
    r = api.Renderer(sc)
    t = dev(rows)
    got = r.query_overlap_capsule(t, 8)
    assert tuple(got) == KEYS and got["object_id"].shape == (len(rows), 8) and got["triangle_id"].shape == (len(rows), 8) and got["count"].shape == (len(rows),)
    check(got, want, labels, name)
    check(got, twin(r, sc, rows), labels, f"{name}, arrays read back")
    assert (to_host(got["count"]) > 0).sum() > len(rows) // 3
    check(r.query_overlap_capsule(t, 8, sort=True), want, labels, f"{name} sorted")
    for K in (1, 4, 8):
        for count in (True, False):
            if K == 8 and count:
                continue
            ref = host.query_overlap_capsule(sc, rows, K, count)
            ref.pop("stack_max")
            out = r.query_overlap_capsule(t, K, count=count)
            assert tuple(out) == tuple(ref)
            check(out, ref, labels, f"{name} K {K} count {count}")
    only = r.query_overlap_capsule(t, 0)
    assert tuple(only) == ("count",)
    check(only, want, labels, f"{name} count only")
    check(r.query_overlap_capsule(t, 0, sort=True), want, labels, f"{name} count only, sorted")
    for K in (8, 1, 0):                                                                     # the objects form
        ref = host.query_overlap_capsule(sc, rows, K, objects=True)
        ref.pop("stack_max")
        for sort in (False, True):
            out = r.query_overlap_capsule(t, K, objects=True, sort=sort)
            assert tuple(out) == tuple(ref) and "triangle_id" not in out
            check(out, ref, labels, f"{name} objects K {K} sort {sort}")
    anyw = host.query_overlapped_capsule(sc, rows)
    assert np.array_equal(anyw, (want["count"] > 0).astype(np.int32))
    for sort in (False, True):
        a = r.query_overlapped_capsule(t, sort=sort)
        assert a.shape == (len(rows),) and np.array_equal(to_host(a), anyw), (name, sort, np.flatnonzero(to_host(a) != anyw)[:8])
    if name == "cube":                                                                       # exact touching, and one ulp off it, on the device
        cnt = to_host(got["count"])
        assert (cnt[capsuleset.in_classes(labels, capsuleset.TOUCHING)] > 0).all() and (cnt[capsuleset.in_classes(labels, ("touch_vertex_off",))] == 0).all()


# ---- 2. batch sizes, rounds, tiles -----------------------------------------------------------------------------------------------------
def answers(sc, rows, blas=None):
    from pyrtx import host
    out = {"list": host.query_overlap_capsule(sc, rows, 8, blas=blas), "objects": host.query_overlap_capsule(sc, rows, 8, objects=True, blas=blas),
           "any": {"count": host.query_overlapped_capsule(sc, rows, blas=blas)}}
    out["stack_max"] = out["list"].pop("stack_max"); out["objects"].pop("stack_max")
    return out


def long_set(name, n):
    """(scene, n rows, labels, twin K = 8 / objects K = 8 / any): generated sets of seeds 4 apart, concatenated and cut; once per run."""
    key = ("long", name, n)
    if key not in _CACHE:
        parts, labs, k = [], [], 0
        while sum(len(p) for p in parts) < n:
            sc, b, lab, _ = generated(name, seed=11 + 4 * k)
            parts.append(b); labs.append(lab); k += 1
        rows = np.ascontiguousarray(np.concatenate(parts)[:n]); labs = np.concatenate(labs)[:n]
        _CACHE[key] = (sc, rows, labs, answers(sc, rows))
    return _CACHE[key]


def run_forms(r, t, sort, n=None):
    return {"list": r.query_overlap_capsule(t, 8, n=n, sort=sort), "objects": r.query_overlap_capsule(t, 8, objects=True, n=n, sort=sort),
            "any": {"count": r.query_overlapped_capsule(t, n=n, sort=sort)}, "count only": {"count": r.query_overlap_capsule(t, 0, n=n, sort=sort)["count"]}}


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
    """2^20 + 3 rows on the cube: mostly far rows, the labelled set at both ends — the second round starts three rows before the end."""
    from pyrtx import host
    sc, rows, labels, want = generated("cube")
    N = api.RTX_QUERY_CHUNK_RAYS + 3
    assert N == (1 << 20) + 3
    far = rows[capsuleset.in_classes(labels, ("far",))]
    big = np.empty((N, 7), f32)
    big[:] = np.resize(far, (N, 7))
    big[:len(rows)] = rows; big[-len(rows):] = rows
    ref_any = host.query_overlapped_capsule(sc, big)
    ref = host.query_overlap_capsule(sc, big, 1)
    assert ref["count"][-3:].any() or ref["count"][-len(rows):].any()
    assert not ref["count"][len(rows):-len(rows)].any()
    r = api.Renderer(sc)
    t = dev(big)
    for sort in (False, True):
        assert np.array_equal(to_host(r.query_overlap_capsule(t, 0, sort=sort)["count"]), ref["count"]), sort
        assert np.array_equal(to_host(r.query_overlapped_capsule(t, sort=sort)), ref_any), sort
    out = r.query_overlap_capsule(t, 1)
    ref.pop("stack_max")
    check(out, ref, None, "2^20 + 3 rows")


def heavy_then_light(name):
    """1100 rows (five tiles): the rows with the most overlaps first (quad_stack: full lists; left_chain: the deepest stacks), the rows that touch
    nothing last: a lane's list, stack and count must not carry over to the row it walks in its next tile."""
    key = ("heavy", name)
    if key not in _CACHE:
        sc, rows, labels, want = long_set(name, 1100)
        order = np.argsort(-want["list"]["count"], kind="stable")
        _CACHE[key] = (sc, np.ascontiguousarray(rows[order]), labels[order], answers(sc, rows[order]))
    return _CACHE[key]


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("name", ["quad_stack", "left_chain"])
def test_later_tiles_carry_nothing_over(api, monkeypatch, name, grid):
    from pyrtx import host
    sc, rows, labels, want = heavy_then_light(name)
    cnt = want["list"]["count"]
    assert (len(rows) + TILE - 1) // TILE >= 5 and (cnt[:TILE] > 0).all() and (cnt[-TILE // 2:] == 0).all()
    if name == "quad_stack":
        assert (cnt[:TILE] > 8).all(), "a tile of full lists, then shorter and empty ones"
    else:
        assert host.query_overlap_capsule(sc, rows[:TILE], 0)["stack_max"] > LDS_STACK, "the spill region, then rows that stay in LDS"
    r = renderer(api, monkeypatch, sc, grid)
    t = dev(rows)
    state, blas = read_back(r, sc)
    back = answers(state, rows, blas)
    for sort in (False, True):
        got = run_forms(r, t, sort)
        compare(got, want, labels, f"{name} grid {grid} sort {sort}")
        compare(got, back, labels, f"{name} grid {grid} sort {sort}, arrays read back")


# ---- 3. consistency with the merged queries, on the device -----------------------------------------------------------------------------
EPS = 1e-3                # far above either side's margin (parts in 10^5 at these scales): a row whose answer survives it is decided on both sides


@pytest.mark.parametrize("name", ["cube", "coincident", "materials_aniso", "quad_stack"])
def test_a_ball_row_is_query_nearest_within_r(api, name):
    sc, rows, labels, want = generated(name)
    r = api.Renderer(sc)
    live = capsuleset.in_classes(labels, capsuleset.NON_TOUCHING)        # the touch classes sit on the decision by construction
    balls = rows[live].copy()
    balls[:, 3:6] = 0.0                                                  # every live row's start point as a ball
    balls[:, 6] = np.maximum(balls[:, 6], f32(1e-3))
    got = to_host(r.query_overlapped_capsule(dev(balls)))
    lo, hi = balls.copy(), balls.copy()
    lo[:, 6] *= f32(1 - EPS); hi[:, 6] *= f32(1 + EPS)
    decided = to_host(r.query_overlapped_capsule(dev(lo))) == to_host(r.query_overlapped_capsule(dev(hi)))
    pts = np.ascontiguousarray(np.concatenate([balls[:, :3], np.full((len(balls), 1), np.inf, f32)], axis=1))
    near = to_host(r.query_nearest(dev(pts), "distance")["distance"])
    compared = int(decided.sum())
    assert compared >= 0.9 * len(balls) and len(balls) > 100, (name, compared, len(balls))
    assert np.array_equal(got[decided] > 0, (near <= balls[:, 6])[decided]), (name, np.flatnonzero(decided & ((got > 0) != (near <= balls[:, 6])))[:8])
    assert 10 < (got > 0).sum() < len(balls)


@pytest.mark.parametrize("name", ["cube", "coincident", "materials_aniso", "quad_stack"])
def test_a_capsule_is_query_sweep_along_its_axis(api, name):
    sc, rows, labels, want = generated(name)
    r = api.Renderer(sc)
    length = np.linalg.norm(rows[:, 3:6].astype(np.float64), axis=1)
    with np.errstate(invalid="ignore"):
        use = capsuleset.in_classes(labels, capsuleset.NON_TOUCHING) & (rows[:, 6] > 0) & (length > 0)
    caps = rows[use]
    L = length[use]
    got = to_host(r.query_overlapped_capsule(dev(caps)))
    lo, hi = caps.copy(), caps.copy()
    lo[:, 3:] *= f32(1 - EPS); hi[:, 3:] *= f32(1 + EPS)              # shorter and thinner, longer and thicker
    decided = to_host(r.query_overlapped_capsule(dev(lo))) == to_host(r.query_overlapped_capsule(dev(hi)))
    sweeps = np.ascontiguousarray(np.concatenate([caps[:, :3], (caps[:, 3:6] / L[:, None]).astype(f32), L[:, None].astype(f32), caps[:, 6:7]], axis=1), f32)
    t = to_host(r.query_sweep(dev(sweeps), "distance")["distance"])
    compared = int(decided.sum())
    assert compared >= 0.8 * len(caps) and len(caps) > 80, (name, compared, len(caps))
    assert np.array_equal(got[decided] > 0, np.isfinite(t)[decided]), (name, np.flatnonzero(decided & ((got > 0) != np.isfinite(t)))[:8])
    assert 10 < (got > 0).sum() < len(caps)


# ---- 4. guards, out= and raw pointers --------------------------------------------------------------------------------------------------
def test_outputs_write_nothing_else(api):
    import torch
    from pyrtx import host
    sc, rows, labels, _ = generated("quad_stack")
    K, n, pad = 3, len(rows), 16
    want = host.query_overlap_capsule(sc, rows, K)
    want_obj = host.query_overlap_capsule(sc, rows, K, objects=True)
    anyw = host.query_overlapped_capsule(sc, rows)
    r = api.Renderer(sc)
    t = dev(rows)

    def sentinels():
        return {"object_id": torch.full((n + pad, K), -77, dtype=torch.int32, device="cuda"), "triangle_id": torch.full((n + pad, K), -77, dtype=torch.int32, device="cuda"),
                "count": torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")}

    def raw(buf, names, m=n, sort=False, **kw):
        torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
        r.query_overlap_capsule(t.data_ptr(), out={k: buf[k].data_ptr() for k in names}, n=m, sort=sort, **kw)
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
    for which in (0, 1):                                                # one id array alone, through the C ABI
        one = sentinels()
        torch.cuda.synchronize()
        assert r.lib.rtx_query_overlap_capsule(r.ctx, t.data_ptr(), n, K, one["object_id"].data_ptr() if which == 0 else None, one["triangle_id"].data_ptr() if which else None, None, 0) == 0
        r.synchronize()
        hit, miss = ("object_id", "triangle_id") if which == 0 else ("triangle_id", "object_id")
        assert np.array_equal(to_host(one[hit][:n]), want[hit]) and bool((one[miss] == -77).all()) and bool((one["count"] == -77).all()) and bool((one[hit][n:] == -77).all())
    av = torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.query_overlapped_capsule(t.data_ptr(), out=av.data_ptr(), n=n)
    r.synchronize()
    assert np.array_equal(to_host(av[:n]), anyw) and bool((av[n:] == -77).all())
    mine = {"object_id": torch.empty((n, K), dtype=torch.int32, device="cuda"), "count": torch.empty((n,), dtype=torch.int32, device="cuda")}
    got = r.query_overlap_capsule(t, K, out=mine)                         # out= tensors are the ones returned
    assert got["object_id"] is mine["object_id"] and got["count"] is mine["count"] and got["triangle_id"].shape == (n, K)
    check(got, want, labels, "out= tensors")
    flag = torch.empty((n,), dtype=torch.int32, device="cuda")
    assert r.query_overlapped_capsule(t, out=flag) is flag and np.array_equal(to_host(flag), anyw)


# ---- 5. sorted rounds with dead and ball rows ------------------------------------------------------------------------------------------
def test_sorted_rounds_answer_row_for_row(api):
    sc, rows, labels, _ = long_set("coincident", 400)
    rng = np.random.default_rng(8)
    rows = rows[rng.permutation(len(rows))].copy()
    rows[::6, 6] = np.nan                                             # planted dead rows
    rows[2::11, 0] = np.inf
    rows[5::13, 6] = -1.0
    rows[7::5, 3:6] = 0.0                                             # balls: no ray key, filed with the dead rows, walked all the same
    r = api.Renderer(sc)
    t = dev(rows)
    for K, count in ((8, True), (1, False), (4, True)):
        ref = twin(r, sc, rows, K, count)
        check(r.query_overlap_capsule(t, K, count=count), ref, None, f"unsorted K {K}")
        srt = r.query_overlap_capsule(t, K, count=count, sort=True)
        check(srt, ref, None, f"sorted K {K}")
    dead = capsuleset.is_dead(rows)
    assert dead.sum() > 80 and (to_host(srt["count"])[dead] == 0).all() and (to_host(srt["object_id"])[dead] == -1).all()
    ball = (rows[:, 3:6] == 0).all(axis=1) & ~dead
    assert ball.sum() > 40 and (to_host(srt["count"])[ball] > 0).any()


# ---- 6. masks --------------------------------------------------------------------------------------------------------------------------
def test_masks_scalar_per_row_and_a_device_table(api):
    import torch
    from pyrtx import host
    sc, rows, labels, _ = long_set("coincident", 2 * TILE + 40)      # mask-0 rows on both sides of a wave boundary and of a tile boundary
    want = host.query_overlap_capsule(sc, rows, 8); want.pop("stack_max")
    n = len(rows)
    M = len(sc.instances) + len(sc.spheres) + len(sc.planes)
    r = api.Renderer(sc)
    t = dev(rows)
    check(r.query_overlap_capsule(t, 8, mask=0xFFFFFFFF), want, labels, "all ones, no table")                  # the identity forms: the filtered kernel, nothing hidden
    ones_t = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    check(r.query_overlap_capsule(t, 8, mask=ones_t, sort=True), want, labels, "all ones per row, sorted")
    z = r.query_overlap_capsule(t, 8, mask=0)
    assert not to_host(z["count"]).any() and (to_host(z["object_id"]) == -1).all() and not to_host(r.query_overlapped_capsule(t, mask=0)).any()
    om = (1 << (np.arange(M) % 4)).astype(np.uint32)
    rm = np.array([(1, 2, 4, 8, 3, 12, 15, 0)[i % 8] for i in range(n)], np.uint32)
    rm[60:68] = 0; rm[TILE - 3:TILE + 3] = 0                          # ... in runs across lane 63 | 64 and across the tile's end
    table_t = torch.from_numpy(om.view(np.int32)).cuda()
    r.set_object_masks(table_t)                                                                                # a device tensor: rtx_update_object_masks
    check(r.query_overlap_capsule(t, 8, mask=0xFFFFFFFF), host.query_overlap_capsule(sc, rows, 8, mask=0xFFFFFFFF, object_masks=om) | {"stack_max": None}, labels, "scalar mask, the table")
    rm_t = torch.from_numpy(rm.view(np.int32)).cuda()
    for sort in (False, True):
        for K, objects in ((8, False), (1, False), (8, True), (0, False)):
            ref = host.query_overlap_capsule(sc, rows, K, objects=objects, mask=rm, object_masks=om); ref.pop("stack_max")
            check(r.query_overlap_capsule(t, K, objects=objects, mask=rm_t, sort=sort), ref, labels, f"row masks K {K} objects {objects} sort {sort}")
        assert np.array_equal(to_host(r.query_overlapped_capsule(t, mask=rm_t, sort=sort)), host.query_overlapped_capsule(sc, rows, mask=rm, object_masks=om))
        ref = host.query_overlap_capsule(sc, rows, 8, mask=5, object_masks=om); ref.pop("stack_max")
        check(r.query_overlap_capsule(t, 8, mask=5, sort=sort), ref, labels, f"scalar mask, sort {sort}")
    got = to_host(r.query_overlap_capsule(t, 8, mask=rm_t)["object_id"])
    for i in range(n):
        ids = got[i][got[i] >= 0]
        assert ((om[ids] & rm[i]) != 0).all(), i
    assert (got[rm == 0] == -1).all()
    check(r.query_overlap_capsule(t, 8), want, labels, "the unfiltered call ignores the table")
    r.set_object_masks(None)
    check(r.query_overlap_capsule(t, 8, mask=rm_t), {k: np.where((rm != 0).reshape((-1,) + (1,) * (want[k].ndim - 1)), want[k], 0 if k == "count" else -1) for k in KEYS}, labels, "table dropped")


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
    rows, labels = capsuleset.generate(moved, 8, seed=42)
    got = r.query_overlap_capsule(dev(rows), 4)
    check(got, twin(r, sc, rows, 4), labels, "after update_instances")
    check(r.query_overlap_capsule(dev(rows), 4, objects=True, sort=True), twin(r, sc, rows, 4, objects=True), labels, "after update_instances, objects, sorted")
    old = api.Renderer(sc).query_overlap_capsule(dev(rows), 4)
    assert not np.array_equal(to_host(old["count"]), to_host(got["count"])), "the poses moved nothing these capsules see"
    assert (to_host(got["count"]) > 0).sum() > len(rows) // 3


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
    rows, labels = capsuleset.generate(state, 8, seed=51)
    rows = rows[np.isfinite(rows).all(axis=1) | (labels == capsuleset.CLASSES.index("dead"))]      # the generator aims at triangles, pad slots among them
    got = r.query_overlap_capsule(dev(rows), 4)
    check(got, twin(r, sc, rows, 4), None, "after build_blas")
    assert (to_host(got["count"]) > 0).sum() > len(rows) // 4
    hot = r.read_blas(0).tri_hot
    pads = np.flatnonzero(np.isnan(hot["position_0"]).any(axis=1) | np.isnan(hot["position_edge_1"]).any(axis=1) | np.isnan(hot["position_edge_2"]).any(axis=1))
    listed = to_host(r.query_overlap_capsule(dev(rows), 8)["triangle_id"])
    assert len(pads) > 0 and not np.isin(listed, pads).any(), "a NaN pad slot overlaps nothing"
    verts = twin_of("padded")[3]
    moved = dev(deform(verts, "wave", seed=21))
    r.refit_blas(0, moved)
    r.update_instances(p, q)
    after = r.query_overlap_capsule(dev(rows), 4, sort=True)
    check(after, twin(r, sc, rows, 4), None, "after refit_blas")
    assert not np.array_equal(to_host(after["triangle_id"]), to_host(got["triangle_id"])), "the refit moved nothing these capsules see"
    del keep


# ---- 8. the frames around a call -------------------------------------------------------------------------------------------------------
def test_a_query_leaves_frames_and_stats_alone(api):
    sc, rows, labels, want = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    first = r.render()
    r.render_async()
    got = r.query_overlap_capsule(dev(rows), 8, sort=True)
    flags = r.query_overlapped_capsule(dev(rows))
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    after = r.render()
    for out in (first, after):
        assert out["stats"] == ref["stats"] and util.bit_exact(out["rgb"], ref["rgb"]) and np.array_equal(out["packed"], ref["packed"])
    check(got, want, labels)
    assert np.array_equal(to_host(flags), (want["count"] > 0).astype(np.int32))


# ---- 9. errors -------------------------------------------------------------------------------------------------------------------------
def test_every_error_code_in_order_and_a_valid_query_after_it(api):
    import torch
    from pyrtx import host
    sc, rows, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(rows)
    t = dev(rows)
    obj_t = torch.full((n, 2), -77, dtype=torch.int32, device="cuda"); tri_t = torch.full((n, 2), -77, dtype=torch.int32, device="cuda")
    cnt_t = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    pp, op, tp, cp = t.data_ptr(), obj_t.data_ptr(), tri_t.data_ptr(), cnt_t.data_ptr()
    OBJ, ANY, SORT = api.RTX_OVERLAP_OBJECTS, api.RTX_OVERLAP_ANY, api.RTX_QUERY_SORT
    call, call_f = lib.rtx_query_overlap_capsule, lib.rtx_query_overlap_capsule_filtered
    torch.cuda.synchronize()
    # (ctx, capsules, n, max_hits, object_id, triangle_id, count, flags)
    cases = [(r.ctx, pp, n, 9, op, tp, cp, 0), (r.ctx, pp, n, -1, op, tp, cp, 0),                                        # max_hits
             (r.ctx, pp, n, 2, op, None, cp, ANY), (r.ctx, pp, n, 0, None, None, cp, ANY | OBJ),                          # ANY needs max_hits == 0 and excludes OBJECTS
             (r.ctx, pp, n, 2, op, tp, cp, OBJ),                                                                          # OBJECTS forbids triangle ids
             (r.ctx, pp, n, 0, None, None, None, 0), (r.ctx, pp, n, 0, op, tp, None, 0), (r.ctx, pp, n, 0, None, None, None, ANY),      # max_hits == 0 needs a count
             (r.ctx, pp, n, 2, None, None, cp, 0), (r.ctx, pp, n, 2, None, None, cp, OBJ),                                # max_hits > 0 needs an id array
             (r.ctx, None, n, 2, op, tp, cp, 0), (r.ctx, pp, 0, 2, op, tp, cp, 0), (r.ctx, pp, -5, 2, op, tp, cp, 0),     # the rows
             (r.ctx, pp, n, 2, op, tp, cp, 1), (r.ctx, pp, n, 2, op, tp, cp, 16), (r.ctx, pp, n, 2, op, tp, cp, 64 | SORT), (r.ctx, pp, n, 2, op, tp, cp, 2048),      # flags
             (None, pp, n, 2, op, tp, cp, 0)]
    for args in cases:
        assert call(*args) == INVALID, args[2:]
    filt = api.RtxQueryFilter(None, 1)
    assert call_f(r.ctx, pp, n, 9, op, tp, cp, 0, C.byref(filt)) == INVALID
    assert call_f(r.ctx, pp, n, 2, op, tp, cp, 0, None) == 0                                 # a NULL filter is the unfiltered call
    empty = api.Renderer(sc, upload=False)
    assert call(empty.ctx, pp, n, 2, op, tp, cp, 0) == STATE
    assert call(empty.ctx, pp, n, 0, None, None, cp, ANY) == STATE
    assert call(empty.ctx, pp, n, 2, op, tp, cp, OBJ) == INVALID                              # the argument checks come first
    assert call(empty.ctx, pp, n, 2, op, tp, cp, 1) == INVALID
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert call(rh.ctx, pp, n, 2, op, tp, cp, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert call(rs.ctx, pp, n, 2, op, tp, cp, 0) == LIMIT                                     # the stack rule of a render call
    chain = chain_blas_scene(); chain.config["stack_size"] = 24                               # the walk's own rule: (-1 + 1) + (22 + 1) = 23 entries
    rc = api.Renderer(chain)
    assert call(rc.ctx, pp, n, 2, op, tp, cp, 0) == 0
    three = copy.deepcopy(chain)
    three.instances = np.concatenate([chain.instances] * 3)
    root = chain.blas[0].nodes[0]
    bxs, centres = [], []
    for k in range(3):
        three.instances["world"][k][3] += 9.0 * k; three.instances["world_inv"][k][3] -= 9.0 * k
        bxs.append(np.concatenate([root["aabb_min"] + (9 * k, 0, 0), root["aabb_max"] + (9 * k, 0, 0)])); centres.append((9.0 * k, 0, 0))
    three.tlas_nodes, three.tlas_indices = host.tlas_build_balanced(np.array(centres, f32), np.array(bxs, f32))
    rt = api.Renderer(three)
    assert call(rt.ctx, pp, n, 2, op, tp, cp, 0) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    assert call(rt.ctx, pp, n, 0, None, None, cp, ANY) == LIMIT and "stack" in lib.rtx_last_error(rt.ctx).decode()
    # a frame with a scaled instance: RTX_ERR_STATE after the checks of a render call and before the walk's own stack rule; accepted again
    # after update_instances has written rigid poses
    import affineset
    rn = api.Renderer(affineset.with_linear(three, [affineset.LINEAR["uniform2"]]))
    rsn = api.Renderer(affineset.with_linear(shallow, [affineset.LINEAR["uniform2"]]))
    assert call(rn.ctx, pp, n, 2, op, tp, cp, 0) == STATE and "rigid" in lib.rtx_last_error(rn.ctx).decode()
    assert call(rn.ctx, pp, n, 0, None, None, cp, ANY) == STATE and call_f(rn.ctx, pp, n, 2, op, tp, cp, 0, C.byref(filt)) == STATE
    assert call(rn.ctx, pp, n, 9, op, tp, cp, 0) == INVALID and call(rsn.ctx, pp, n, 2, op, tp, cp, 0) == LIMIT
    scaled = api.Renderer(affineset.with_linear(sc, [affineset.LINEAR["uniform2"]]))
    assert call(scaled.ctx, pp, n, 2, op, tp, cp, 0) == STATE
    ni = len(sc.instances)
    pos = np.stack([np.asarray(m, f32).reshape(4, 4)[:3, 3] for m in sc.instances["world"]]).astype(f32)
    rot = np.tile(f32([0, 0, 0, 1]), (ni, 1))
    p_t, q_t = dev(pos), dev(rot)
    scaled.update_instances(p_t, q_t)
    assert call(scaled.ctx, pp, n, 2, op, tp, cp, 0) == 0
    scaled.synchronize()
    ref = twin(scaled, sc, rows, 2)
    assert np.array_equal(to_host(obj_t), ref["object_id"]) and np.array_equal(to_host(tri_t), ref["triangle_id"]) and np.array_equal(to_host(cnt_t), ref["count"])
    # the state rule of the filtered call comes last: a table set for other counts than the frame's
    r.set_object_masks(np.full(len(sc.instances) + len(sc.spheres) + len(sc.planes), 1, np.uint32))
    fewer = copy.deepcopy(sc); fewer.spheres = fewer.spheres[:-1]
    r.set_frame(fewer)
    assert call_f(r.ctx, pp, n, 2, op, tp, cp, 0, C.byref(filt)) == STATE
    assert call_f(r.ctx, pp, n, 2, op, tp, cp, 2048, C.byref(filt)) == INVALID
    assert call(r.ctx, pp, n, 2, op, tp, cp, 0) == 0                                          # the unfiltered call does not look at the table
    r.set_frame(sc)
    r.set_object_masks(None)
    for other in (empty, rh, rs, rc, rt, rn, rsn, scaled):
        other.synchronize()
    r.synchronize()
    obj_t.fill_(-77); tri_t.fill_(-77); cnt_t.fill_(-77)
    torch.cuda.synchronize()
    for args in cases[:-1]:                                                   # an error queues nothing
        call(*args)
    r.synchronize()
    assert bool((obj_t == -77).all()) and bool((tri_t == -77).all()) and bool((cnt_t == -77).all())
    check(r.query_overlap_capsule(t, 8), want, labels, "after the errors")
