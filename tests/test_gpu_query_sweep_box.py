"""rtx_query_sweep_box on the GPU: rows in device tensors, t, the contact normal, the ids and the axis code in device tensors, bit for bit
against the host twin (host.query_sweep_box, the same code of csrc/rtx_boxsweep_math.h) run on the arrays read back from the context:
  * the row classes of tests/boxsweepset.py over six scenes, two of them chain meshes whose ordered descent reaches the spill region, with
    rows whose D lies one ulp below and above their contact and, on the cube, grazing passes at 4, 16 and 256 bounds either side;
    sorted and unsorted, each output alone and all together, raw pointers;
  * batch sizes around a wave and a workgroup, one call of 2^20 + 3 rows, RTX_QUERY_GRID=1: hard rows, dead tiles, hard rows;
  * scalar, per-row and device-table masks; after update_instances, build_blas and refit_blas;
  * cross-checks on the device with no host twin: a point box against query_closest, t == 0 against query_overlapped, cubes between the
    circumscribed and the inscribed ball of query_sweep, each row under its own bounds over its own cos of incidence;
  * frames and rtx_get_stats unchanged; every error code in the documented order, then a valid call."""
import copy
import ctypes as C

import numpy as np
import pytest

import boxset
import boxsweepset as bs
import hitset
import util
from test_gpu_query import dev, host as to_host
from test_gpu_query_overlap import left_chain_scene, read_back, renderer
from test_gpu_rays import chain_blas_scene, many_instances_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
TILE, LDS_STACK = 256, 16
ALL = ("distance", "normal", "object_id", "triangle_id", "axis")
SCENES = ["cube", "coincident", "materials_aniso", "chain_blas", "left_chain", "many_instances"]
_CACHE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def load_scene(name):
    if name not in _CACHE:
        _CACHE[name] = (chain_blas_scene() if name == "chain_blas" else left_chain_scene() if name == "left_chain" else many_instances_scene() if name == "many_instances" else
                        util.load_golden(name)[0])
    return _CACHE[name]


def twin(r, sc, rows, channels=ALL, mask=None, object_masks=None):
    from pyrtx import host
    state, blas = read_back(r, sc)
    out = host.query_sweep_box(state, rows, channels, blas=blas, mask=mask, object_masks=object_masks)
    out.pop("stack_max")
    return out


def generated(name, seed=7, n=10):
    """(scene, rows, labels, host answers from the scene's own arrays), once per run."""
    key = ("set", name, seed, n)
    if key not in _CACHE:
        from pyrtx import host
        sc = load_scene(name)
        rows, lab = bs.generate(sc, n, seed)
        if name in ("chain_blas", "left_chain"):                           # the rows that fill the stack
            rows = np.concatenate([rows, bs.chain_rows()]); lab = np.concatenate([lab, np.full(12, bs.CLASSES.index("approach"))])
        first = host.query_sweep_box(sc, rows, "distance")["distance"]
        pos = np.flatnonzero(np.isfinite(first) & (first > 0))[:12]          # D just below the contact (no answer, or a later one) and just above it (the same answer)
        below, above = bs.d_rows(rows[pos], first[pos])
        rows = np.concatenate([rows, below, above]); lab = np.concatenate([lab, np.full(len(pos), bs.CLASSES.index("d_below")), np.full(len(pos), bs.CLASSES.index("d_above"))])
        if name == "cube":                                                   # grazing passes: clear of the face x = 1 by 4, 16, 256 bounds, and biting by as much
            B = host.sweep_box_bound(8.0, 0.0, 6.0, 1.0)
            rows = np.concatenate([rows, bs.graze_rows([4 * B, 16 * B, 256 * B, -4 * B, -16 * B, -256 * B])])
            lab = np.concatenate([lab, np.full(3, bs.CLASSES.index("graze_miss")), np.full(3, bs.CLASSES.index("graze_hit"))])
        want = host.query_sweep_box(sc, rows, ALL)
        assert np.array_equal(want["distance"][lab == bs.CLASSES.index("d_above")], first[pos]) and not (want["distance"][lab == bs.CLASSES.index("d_below")] <= first[pos]).any()
        if name == "cube":
            assert np.isinf(want["distance"][lab == bs.CLASSES.index("graze_miss")]).all() and (want["axis"][lab == bs.CLASSES.index("graze_hit")] == 1).all()
        _CACHE[key] = (sc, np.ascontiguousarray(rows), lab, want)
    return _CACHE[key]


def long_set(name, n):
    key = ("long", name, n)
    if key not in _CACHE:
        from pyrtx import host
        parts, labs, k = [], [], 0
        while sum(len(p) for p in parts) < n:
            sc, b, lab, _ = generated(name, seed=11 + 4 * k)
            parts.append(b); labs.append(lab); k += 1
        rows = np.ascontiguousarray(np.concatenate(parts)[:n]); labs = np.concatenate(labs)[:n]
        _CACHE[key] = (sc, rows, labs, host.query_sweep_box(sc, rows, ALL))
    return _CACHE[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check(got, want, labels=None, what=""):
    """Every array of `got` equal to want's bit for bit (a float as its 32 bits); names the outputs and the row classes that differ."""
    bad = {}
    for name, g in got.items():
        g = to_host(g) if hasattr(g, "cpu") else g
        ok = (bits(g) == bits(want[name][:len(g)])).reshape(len(g), -1).all(axis=1)
        if not ok.all():
            rows = np.flatnonzero(~ok)
            bad[name] = (len(rows), rows[:6].tolist(), {} if labels is None else {bs.CLASSES[c]: int((labels[rows] == c).sum()) for c in np.unique(labels[rows])})
    assert not bad, (what, bad)


# ---- 1. parity with the host twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_the_host_walk(api, name):
    sc, rows, labels, want = generated(name)
    assert 100 <= len(rows) <= 300
    if name in ("chain_blas", "left_chain"):
        assert want["stack_max"] > LDS_STACK, "this scene is here to reach the spill region"
    r = api.Renderer(sc)
    t = dev(rows)
    got = r.query_sweep_box(t, ALL)
    assert tuple(got) == ALL and got["distance"].shape == (len(rows),) and got["normal"].shape == (len(rows), 3) and got["axis"].shape == (len(rows),)
    check(got, want, labels, name)
    check(got, twin(r, sc, rows), labels, f"{name}, arrays read back")
    d = to_host(got["distance"])
    assert np.isfinite(d).sum() > len(rows) // 3 and (d == 0).any() and ((d > 0) & np.isfinite(d)).any()
    check(r.query_sweep_box(t, ALL, sort=True), want, labels, f"{name} sorted")
    for ch in ALL:                                                         # each output alone
        for sort in (False, True):
            one = r.query_sweep_box(t, ch, sort=sort)
            assert tuple(one) == (ch,)
            check(one, want, labels, f"{name} {ch} alone, sort {sort}")
    nrm = to_host(got["normal"]).astype(np.float64)
    hit = np.isfinite(d) & (d > 0)
    assert np.allclose(np.linalg.norm(nrm[hit], axis=1), 1.0, atol=1e-5) and not nrm[~hit].any()
    assert ((nrm[hit] * rows[hit, 3:6]).sum(axis=1) <= 1e-6 * np.linalg.norm(rows[hit, 3:6], axis=1)).all(), "a normal that does not oppose the motion"


# ---- 2. batch sizes, rounds, tiles -----------------------------------------------------------------------------------------------------
def test_batch_sizes_around_a_wave_and_a_workgroup(api):
    sc, rows, labels, want = long_set("materials_aniso", 300)
    r = api.Renderer(sc)
    t = dev(rows)
    for n in (1, 63, 64, 65, 255, 256, 257):
        for sort in (False, True):
            got = r.query_sweep_box(t, ALL, n=n, sort=sort)
            assert all(len(x) == n for x in got.values())
            check(got, want, labels, f"n {n} sort {sort}")


def test_one_call_crosses_a_round(api):
    import torch
    sc, rows, labels, want = long_set("cube", 300)
    r = api.Renderer(sc)
    small = dev(rows)
    got = r.query_sweep_box(small, ALL)
    check(got, want, labels, "the small call")
    N = api.RTX_QUERY_CHUNK_RAYS + 3
    assert N == 2 ** 20 + 3
    reps = (N + len(rows) - 1) // len(rows)
    big = small.repeat(reps, 1)[:N].contiguous()
    for sort in (False, True):
        out = r.query_sweep_box(big, ALL, sort=sort)
        for k in ALL:
            ref = got[k].repeat(*((reps,) + (1,) * (got[k].dim() - 1)))[:N]
            same = torch.equal(out[k].view(torch.int32), ref.view(torch.int32))
            assert same, (k, sort)


def test_one_workgroup_walks_hard_rows_dead_tiles_hard_rows(api, monkeypatch):
    sc, rows, labels, want = long_set("chain_blas", 600)
    rows = rows.copy(); rows[:2 * TILE:2] = bs.chain_rows(TILE)            # every other hard row fills the stack into the spill region
    hard = np.arange(2 * TILE)
    dead = np.zeros((2 * TILE, 14), f32); dead[:, 7:10] = 1.0; dead[:, 13] = 1.0; dead[:, 6] = 1.0      # zero direction: dead
    dead[1::3, 3] = np.nan; dead[2::3, 4] = 1.0; dead[2::3, 10:] = 0.0                                  # ... a NaN, a zero quaternion
    assert bs.is_dead(dead).all()
    perm = np.ascontiguousarray(np.concatenate([rows[hard[:TILE]], dead, rows[hard[TILE:]], rows[:77]]))
    from pyrtx import host
    ref = host.query_sweep_box(sc, perm, ALL)
    assert ref["stack_max"] > LDS_STACK and not np.isfinite(ref["distance"][TILE:3 * TILE]).any() and (ref["axis"][TILE:3 * TILE] == -1).all()
    for grid in (1, None):
        r = renderer(api, monkeypatch, sc, grid)
        for sort in (False, True):
            check(r.query_sweep_box(dev(perm), ALL, sort=sort), ref, None, f"grid {grid} sort {sort}")


def test_sorted_rounds_with_dead_rows(api):
    sc, rows, labels, _ = long_set("coincident", 400)
    rng = np.random.default_rng(8)
    rows = rows[rng.permutation(len(rows))].copy()
    rows[::6, 13] = np.nan
    rows[2::11, 0] = np.inf
    rows[5::13, 8] = -1.0
    rows[3::17, 3:6] = 0.0
    rows[4::19, 6] = 0.0
    r = api.Renderer(sc)
    ref = twin(r, sc, rows)
    check(r.query_sweep_box(dev(rows), ALL), ref, None, "unsorted")
    srt = r.query_sweep_box(dev(rows), ALL, sort=True)
    check(srt, ref, None, "sorted")
    dead = bs.is_dead(rows)
    assert dead.sum() > 100 and np.isinf(to_host(srt["distance"])[dead]).all() and (to_host(srt["object_id"])[dead] == -1).all() and (to_host(srt["axis"])[dead] == -1).all()


# ---- 3. guards, out= and raw pointers --------------------------------------------------------------------------------------------------
def test_raw_pointers_and_out_tensors_write_nothing_else(api):
    import torch
    sc, rows, labels, want = generated("materials_aniso")
    n, pad = len(rows), 16
    r = api.Renderer(sc)
    t = dev(rows)

    def sentinels():
        return {"distance": torch.full((n + pad,), -77.0, device="cuda"), "normal": torch.full((n + pad, 3), -77.0, device="cuda"),
                "object_id": torch.full((n + pad,), -77, dtype=torch.int32, device="cuda"), "triangle_id": torch.full((n + pad,), -77, dtype=torch.int32, device="cuda"),
                "axis": torch.full((n + pad,), -77, dtype=torch.int32, device="cuda")}

    for sort in (False, True):
        for names, m in ((ALL, n), (ALL, n - 5), (("distance", "axis"), n), (("normal",), n)):
            buf = sentinels()
            torch.cuda.synchronize()                                        # raw pointers: the work goes to the context's stream, not torch's
            r.query_sweep_box(t.data_ptr(), names, out={k: buf[k].data_ptr() for k in names}, n=m, sort=sort)
            r.synchronize()
            check({k: buf[k][:m] for k in names}, want, labels, f"raw pointers {names} n {m} sort {sort}")
            for k, v in buf.items():
                assert bool((v[m:] == -77).all()) and (k in names or bool((v == -77).all())), (k, names, m, sort)
    mine = {"distance": torch.empty((n,), device="cuda"), "axis": torch.empty((n,), dtype=torch.int32, device="cuda")}
    got = r.query_sweep_box(t, ALL, out=mine)
    assert got["distance"] is mine["distance"] and got["axis"] is mine["axis"]
    check(got, want, labels, "out= tensors")


# ---- 4. masks --------------------------------------------------------------------------------------------------------------------------
def test_masks_scalar_per_row_and_a_device_table(api):
    import torch
    from pyrtx import host
    sc, rows, labels, want = generated("coincident")
    n = len(rows)
    M = len(sc.instances) + len(sc.spheres) + len(sc.planes)
    r = api.Renderer(sc)
    t = dev(rows)
    check(r.query_sweep_box(t, ALL, mask=0xFFFFFFFF), want, labels, "all ones, no table")
    z = r.query_sweep_box(t, ALL, mask=0)
    assert np.isinf(to_host(z["distance"])).all() and (to_host(z["object_id"]) == -1).all() and (to_host(z["axis"]) == -1).all() and not to_host(z["normal"]).any()
    om = (1 << (np.arange(M) % 4)).astype(np.uint32)
    rm = np.array([(1, 2, 4, 8, 3, 12, 15, 0)[i % 8] for i in range(n)], np.uint32)
    r.set_object_masks(torch.from_numpy(om.view(np.int32)).cuda())
    rm_t = torch.from_numpy(rm.view(np.int32)).cuda()
    for sort in (False, True):
        ref = host.query_sweep_box(sc, rows, ALL, mask=rm, object_masks=om); ref.pop("stack_max")
        got = r.query_sweep_box(t, ALL, mask=rm_t, sort=sort)
        check(got, ref, labels, f"row masks sort {sort}")
        ref5 = host.query_sweep_box(sc, rows, ALL, mask=5, object_masks=om); ref5.pop("stack_max")
        check(r.query_sweep_box(t, ALL, mask=5, sort=sort), ref5, labels, f"scalar mask sort {sort}")
    ids = to_host(got["object_id"])
    assert ((om[ids[ids >= 0]] & rm[ids >= 0]) != 0).all() and (ids != want["object_id"]).any()
    check(r.query_sweep_box(t, ALL), want, labels, "the unfiltered call ignores the table")
    r.set_object_masks(None)


# ---- 5. device-side scene changes ------------------------------------------------------------------------------------------------------
def test_after_update_instances(api):
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
    rows, labels = bs.generate(moved, 8, seed=42)
    got = r.query_sweep_box(dev(rows), ALL)
    check(got, twin(r, sc, rows), labels, "after update_instances")
    check(r.query_sweep_box(dev(rows), ALL, sort=True), twin(r, sc, rows), labels, "after update_instances, sorted")
    old = api.Renderer(sc).query_sweep_box(dev(rows), "distance")
    assert not np.array_equal(to_host(old["distance"]), to_host(got["distance"])), "the poses moved nothing these rows see"
    assert np.isfinite(to_host(got["distance"])).sum() > len(rows) // 3


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
    rows, labels = bs.generate(state, 8, seed=51)
    rows = rows[np.isfinite(rows[:, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13]]).all(axis=1) | (labels == bs.CLASSES.index("dead"))]      # the generator aims at triangles, pad slots among them
    got = r.query_sweep_box(dev(rows), ALL)
    check(got, twin(r, sc, rows), None, "after build_blas")
    assert np.isfinite(to_host(got["distance"])).sum() > len(rows) // 4
    hot = r.read_blas(0).tri_hot
    pads = np.flatnonzero(np.isnan(hot["position_0"]).any(axis=1) | np.isnan(hot["position_edge_1"]).any(axis=1) | np.isnan(hot["position_edge_2"]).any(axis=1))
    assert len(pads) > 0 and not np.isin(to_host(got["triangle_id"]), pads).any(), "a NaN pad slot stops nothing"
    verts = twin_of("padded")[3]
    r.refit_blas(0, dev(deform(verts, "wave", seed=21)))
    r.update_instances(p, q)
    after = r.query_sweep_box(dev(rows), ALL, sort=True)
    check(after, twin(r, sc, rows), None, "after refit_blas")
    assert not np.array_equal(to_host(after["distance"]), to_host(got["distance"])), "the refit moved nothing these rows see"
    del keep


# ---- 6. cross-checks on the device, no host twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "materials_aniso"])
def test_device_cross_checks(api, name):
    from pyrtx import host
    sc, rows, labels, want = generated(name)
    r = api.Renderer(sc)
    live = ~bs.is_dead(rows)
    lo, hi = hitset.world_box(sc)
    diag = float(np.linalg.norm(hi - lo))
    # a point box is a ray: its t against query_closest's distance on the same rays.  Per row, on triangle answers both name, where the returned
    # normal is within COS_FLOOR of the motion and the bound does not exclude the contact: |t_box - t_ray| |d| <= sweep_box_bound(S, W, T, kappa
    # of the winning axis) / cos + the hit test's own margin in t, S, W and kappa the row's own at its contact (tests/boxsweepset.py contact())
    pts = rows[live].copy(); pts[:, 7:10] = 0.0; pts[:, 6] = np.inf
    pt = {k: to_host(v) for k, v in r.query_sweep_box(dev(pts), ALL).items()}
    cl = {k: to_host(v) for k, v in r.query_closest(dev(np.ascontiguousarray(pts[:, :6])), ("distance", "object_id")).items()}
    dl = np.linalg.norm(pts[:, 3:6].astype(np.float64), axis=1)
    ni = len(sc.instances)
    starts_on = pt["distance"] <= 0.01                                     # a centre that starts on or just off a surface: the ray kernels take no hit at t <= 0.005 (RAY_EPSILON)
    compared = 0
    for i in np.flatnonzero(np.isfinite(pt["distance"]) & np.isfinite(cl["distance"]) & ~starts_on & (pt["object_id"] >= 0) & (pt["object_id"] < ni) & (cl["object_id"] < ni)):
        t = float(pt["distance"][i])
        S, W, kap, k, cos, excluded, sliver, gap = bs.contact(sc, pts[i], t, int(pt["object_id"][i]), int(pt["triangle_id"][i]), pt["normal"][i])
        if excluded or cos < bs.COS_FLOOR or sliver > 4:
            continue
        S0 = bs.contact(sc, pts[i], 0.0, int(pt["object_id"][i]), int(pt["triangle_id"][i]), pt["normal"][i])[0]
        bound = host.sweep_box_bound(S, W, t * dl[i], kap) / cos + host.hits_margin(sliver / cos, (S0 + 8 * W) / dl[i]) * dl[i]
        assert abs(t - float(cl["distance"][i])) * dl[i] <= bound, (name, i, t, float(cl["distance"][i]), bound, k, kap, cos)
        compared += 1
    assert compared > len(pts) // 4, compared
    one_sided = (np.isfinite(pt["distance"]) != np.isfinite(cl["distance"])) & ~starts_on
    assert one_sided.sum() <= len(pts) // 20, "rays that graze an edge may differ; more than that may not"
    # t == 0 iff query_overlapped says so, on rows with clearance (the generated classes keep clear of touching, `touch` and `parallel` apart)
    clear = live & ~bs.in_classes(labels, ("touch", "parallel", "sphere_cross", "edge_edge", "graze_hit", "graze_miss"))
    ov = to_host(r.query_overlapped(dev(bs.box_of(rows))))
    t = to_host(r.query_sweep_box(dev(rows), "distance")["distance"])
    far_enough = clear & ((rows[:, 6] > 0) & np.isfinite(rows[:, :6]).all(axis=1))
    assert np.array_equal((t == 0)[far_enough], ov[far_enough] == 1), (name, np.flatnonzero(far_enough & ((t == 0) != (ov == 1)))[:8])
    assert (t == 0)[far_enough].sum() >= 4
    # cubes: between the circumscribed and the inscribed ball of query_sweep, within both bounds.  Per row: the box's bound at its own contact, the
    # ball's sweep_bound at the ball's contact (S = its radius + the mesh's longest edge twice), each divided by |d| cos of its own contact normal;
    # rows where either normal is beyond COS_FLOOR of the motion, or the box's contact is one its bound excludes, are skipped
    cubes = rows[live & bs.in_classes(labels, ("approach", "face_on", "vertex_face", "d_inf", "edge_edge"))].copy()
    cubes[:, 7:10] = cubes[:, 7:8]; cubes[:, 6] = np.inf
    cubes = cubes[cubes[:, 7] > 0]
    box = {k: to_host(v) for k, v in r.query_sweep_box(dev(cubes), ALL).items()}
    tb = box["distance"]
    emax = max(float(max(np.linalg.norm(b.tri_hot["position_edge_1"], axis=1).max(), np.linalg.norm(b.tri_hot["position_edge_2"], axis=1).max(),
                         np.linalg.norm(b.tri_hot["position_edge_2"] - b.tri_hot["position_edge_1"], axis=1).max())) for b in sc.blas)
    dl = np.linalg.norm(cubes[:, 3:6].astype(np.float64), axis=1)

    def ball(radius):
        sw = np.ascontiguousarray(np.concatenate([cubes[:, :7], radius[:, None]], axis=1).astype(f32))
        o = {k: to_host(v) for k, v in r.query_sweep(dev(sw), ("distance", "position")).items()}
        slack = np.full(len(sw), np.nan)
        for i in np.flatnonzero(np.isfinite(o["distance"]) & (o["distance"] > 0)):
            c = sw[i, :3].astype(np.float64) + float(o["distance"][i]) * sw[i, 3:6].astype(np.float64)
            n = c - o["position"][i].astype(np.float64)
            cos = abs(float(n @ sw[i, 3:6])) / (float(np.linalg.norm(n)) * dl[i]) if np.linalg.norm(n) > 0 else 0.0
            if cos >= bs.COS_FLOOR:
                slack[i] = host.sweep_bound(float(radius[i]) + 2 * emax, bs.world_scale(sc, c), float(o["distance"][i]) * dl[i], float(radius[i])) / (cos * dl[i])
        return o["distance"], slack
    (outer, so), (inner, si) = ball(cubes[:, 7] * f32(np.sqrt(3.0))), ball(cubes[:, 7].copy())
    lower = upper = 0
    for i in np.flatnonzero(np.isfinite(tb) & (tb > 0) & (box["object_id"] >= 0) & (box["object_id"] < ni)):
        t = float(tb[i])
        S, W, kap, k, cos, excluded, _, _ = bs.contact(sc, cubes[i], t, int(box["object_id"][i]), int(box["triangle_id"][i]), box["normal"][i])
        if excluded or cos < bs.COS_FLOOR:
            continue
        sb = host.sweep_box_bound(S, W, t * dl[i], kap) / (cos * dl[i])
        if np.isfinite(so[i]):
            assert outer[i] <= t + sb + so[i], (name, i, float(outer[i]), t, sb, so[i]); lower += 1
        if np.isfinite(si[i]):
            assert t <= inner[i] + sb + si[i], (name, i, t, float(inner[i]), sb, si[i]); upper += 1
    assert len(cubes) >= 16 and lower >= 10 and upper >= 10, (len(cubes), lower, upper)
    assert (outer < tb).any() and (tb < inner).any()


# ---- 7. the frames around a call; errors -----------------------------------------------------------------------------------------------
def test_a_query_leaves_frames_and_stats_alone(api):
    sc, rows, labels, want = generated("materials_aniso")
    ref = api.Renderer(sc).render()
    r = api.Renderer(sc)
    first = r.render()
    r.render_async()
    got = r.query_sweep_box(dev(rows), ALL, sort=True)
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"])
    after = r.render()
    for out in (first, after):
        assert out["stats"] == ref["stats"] and util.bit_exact(out["rgb"], ref["rgb"]) and np.array_equal(out["packed"], ref["packed"])
    check(got, want, labels)


def test_every_error_code_in_order_and_a_valid_query_after_it(api):
    import torch
    from pyrtx import host
    sc, rows, labels, want = generated("materials_aniso")
    r = api.Renderer(sc)
    lib, n = r.lib, len(rows)
    t = dev(rows)
    t_t = torch.full((n,), -77.0, device="cuda"); n_t = torch.full((n, 3), -77.0, device="cuda")
    o_t, s_t, a_t = (torch.full((n,), -77, dtype=torch.int32, device="cuda") for _ in range(3))
    pp, tp, np_, op, sp, ap = t.data_ptr(), t_t.data_ptr(), n_t.data_ptr(), o_t.data_ptr(), s_t.data_ptr(), a_t.data_ptr()
    SORT = api.RTX_QUERY_SORT
    torch.cuda.synchronize()
    # (ctx, sweeps, n, t, normal, object_id, triangle_id, axis, flags)
    cases = [(r.ctx, None, n, tp, np_, op, sp, ap, 0), (r.ctx, pp, n, None, None, None, None, None, 0), (r.ctx, pp, 0, tp, np_, op, sp, ap, 0), (r.ctx, pp, -5, tp, np_, op, sp, ap, 0),
             (r.ctx, pp, n, tp, np_, op, sp, ap, 1), (r.ctx, pp, n, tp, np_, op, sp, ap, 64 | SORT), (r.ctx, pp, n, tp, np_, op, sp, ap, 512), (r.ctx, pp, n, tp, np_, op, sp, ap, 1024),
             (None, pp, n, tp, np_, op, sp, ap, 0)]
    for args in cases:
        assert lib.rtx_query_sweep_box(*args) == INVALID, args[2:]
    filt = api.RtxQueryFilter(None, 1)
    assert lib.rtx_query_sweep_box_filtered(r.ctx, pp, n, None, None, None, None, None, 0, C.byref(filt)) == INVALID
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_query_sweep_box(empty.ctx, pp, n, tp, None, None, None, None, 0) == STATE
    assert lib.rtx_query_sweep_box(empty.ctx, pp, n, tp, None, None, None, None, 1) == INVALID          # the argument checks come first
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert lib.rtx_query_sweep_box(rh.ctx, pp, n, tp, np_, op, sp, ap, 0) == STATE
    shallow, _ = util.load_golden("monkey_small"); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert lib.rtx_query_sweep_box(rs.ctx, pp, n, tp, np_, op, sp, ap, 0) == LIMIT
    chain = chain_blas_scene(); chain.config["stack_size"] = 24
    rc = api.Renderer(chain)
    assert lib.rtx_query_sweep_box(rc.ctx, pp, n, tp, np_, op, sp, ap, 0) == 0
    three = copy.deepcopy(chain)
    three.instances = np.concatenate([chain.instances] * 3)
    root = chain.blas[0].nodes[0]
    bxs, centres = [], []
    for k in range(3):
        three.instances["world"][k][3] += 9.0 * k; three.instances["world_inv"][k][3] -= 9.0 * k
        bxs.append(np.concatenate([root["aabb_min"] + (9 * k, 0, 0), root["aabb_max"] + (9 * k, 0, 0)])); centres.append((9.0 * k, 0, 0))
    three.tlas_nodes, three.tlas_indices = host.tlas_build_balanced(np.array(centres, f32), np.array(bxs, f32))
    rt = api.Renderer(three)
    assert lib.rtx_query_sweep_box(rt.ctx, pp, n, tp, np_, op, sp, ap, 0) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    # a frame with a scaled instance: RTX_ERR_STATE after the checks of a render call (a shallow stack stays RTX_ERR_LIMIT) and before the walk's
    # own stack rule (the three chains, enlarged by 2, are no longer RTX_ERR_LIMIT); the argument checks still come first; nothing is queued
    import affineset
    rn = api.Renderer(affineset.with_linear(three, [affineset.LINEAR["uniform2"]]))
    rsn = api.Renderer(affineset.with_linear(shallow, [affineset.LINEAR["uniform2"]]))
    assert lib.rtx_query_sweep_box(rn.ctx, pp, n, tp, np_, op, sp, ap, 0) == STATE and "rigid" in lib.rtx_last_error(rn.ctx).decode()
    assert lib.rtx_query_sweep_box_filtered(rn.ctx, pp, n, tp, np_, op, sp, ap, 0, C.byref(filt)) == STATE
    assert lib.rtx_query_sweep_box(rn.ctx, pp, n, tp, np_, op, sp, ap, 1) == INVALID and lib.rtx_query_sweep_box(rsn.ctx, pp, n, tp, np_, op, sp, ap, 0) == LIMIT
    rn.synchronize(); rsn.synchronize()
    assert "stack" in lib.rtx_last_error(rt.ctx).decode()
    r.set_object_masks(np.full(len(sc.instances) + len(sc.spheres) + len(sc.planes), 1, np.uint32))
    fewer = copy.deepcopy(sc); fewer.spheres = fewer.spheres[:-1]
    r.set_frame(fewer)
    assert lib.rtx_query_sweep_box_filtered(r.ctx, pp, n, tp, np_, op, sp, ap, 0, C.byref(filt)) == STATE      # the state rule of the filtered call comes last
    assert lib.rtx_query_sweep_box_filtered(r.ctx, pp, n, tp, np_, op, sp, ap, 2048, C.byref(filt)) == INVALID
    assert lib.rtx_query_sweep_box(r.ctx, pp, n, tp, np_, op, sp, ap, 0) == 0
    r.set_frame(sc)
    r.set_object_masks(None)
    for other in (empty, rh, rs, rc, rt):
        other.synchronize()
    r.synchronize()
    for x in (t_t, n_t, o_t, s_t, a_t):
        x.fill_(-77)
    torch.cuda.synchronize()
    for args in cases[:-1]:                                                   # an error queues nothing
        lib.rtx_query_sweep_box(*args)
    r.synchronize()
    assert all(bool((x == -77).all()) for x in (t_t, n_t, o_t, s_t, a_t))
    check(r.query_sweep_box(t, ALL), want, labels, "after the errors")
