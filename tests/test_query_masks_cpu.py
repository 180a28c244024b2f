"""The filtered walk queries on the host (host.query_nearest / query_hits / query_sweep with mask= and object_masks=: rtxh_query_*_filtered,
the code the filtered kernels compile), no GPU:
  * each filtered twin against its filtered exhaustive search under its header's own promise: nearest never nearer and farther by at most
    rtxh_nearest_distance_bound of the exhaustive winner; every listed hit a hit of the exhaustive search with the same bits and the count
    never above; the sweep never earlier, bit-equal where the time is, and ACCURACY's property (rtxh_sweep_bound) in fp64 against the
    scene with the hidden objects removed;
  * the filtered nearest answer against the UNFILTERED twin on a scene from which the hidden objects were really removed (another TLAS, so
    other bits are allowed: distances within the bound of the winner);
  * no answer names a hidden object; rows of mask 0 get the no-answer record; the stack stays within stack_need;
  * the identity forms (no table with all ones, a table of all ones with rows of all ones) are the unfiltered answers bit for bit;
  * two coincident instances with disjoint masks: the one the row sees is reported;
  * against vacuous passes: in every scene some row's answer differs from the unfiltered one and some row's does not;
  * csrc/mask_check.cpp under the host sanitizers; declarations, exports and the Python layer's checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import hitset
import maskset
import pointset
import sweepset
import util
import test_query_hits_cpu as HC
import test_query_nearest_cpu as NC
import test_query_sweep_cpu as SC
from test_gpu_rays import chain_blas_scene, many_instances_scene

f32 = np.float32
u32 = np.uint32
REPO = util.REPO
ALL = hitset.ALL
ONES = maskset.ALL_ONES
# scene -> (seed of the object masks, seed of the row masks): chosen with the host twin so that every kind has rows the filter changes and rows it
# does not (test_the_filter_changes_some_rows_and_not_others)
SEEDS = {"many_instances": (3, 7), "coincident": (0, 5), "cube": (2, 9), "materials_aniso": (4, 11)}
_CACHE = {}


@pytest.fixture(scope="module")
def host():
    from pyrtx import host as h
    h.lib()
    return h


def load_scene(name):
    if name == "chain_blas":
        return chain_blas_scene()
    if name == "many_instances":
        return many_instances_scene()
    return util.load_golden(name)[0]


def table_of(name, sc):
    return maskset.coincident_masks(sc) if name == "coincident" else maskset.object_masks(sc, SEEDS[name][0])


def rows_of(kind, name, sc):
    if kind == "nearest":
        return pointset.generate(sc, 160, seed=13)[0][:320]
    if kind == "hits":
        return hitset.generate(sc, 14, seed=13)[0][:320]
    return sweepset.generate(sc, 160, seed=13)[0][:320]


def case(host, kind, name):
    """(scene, rows, object masks, row masks, filtered walk, filtered exhaustive, unfiltered walk), once per run; hits at K = 8 with the count."""
    key = (kind, name)
    if key not in _CACHE:
        sc = load_scene(name)
        rows = np.ascontiguousarray(rows_of(kind, name, sc))
        table, rm = table_of(name, sc), maskset.row_masks(len(rows), SEEDS[name][1])
        if kind == "nearest":
            w = host.query_nearest(sc, rows, ALL, mask=rm, object_masks=table)
            e = host.query_nearest_exhaustive(sc, rows, ALL, mask=rm, object_masks=table)
            u = host.query_nearest(sc, rows, ALL)
        elif kind == "hits":
            w = host.query_hits(sc, rows, 8, ALL, mask=rm, object_masks=table)
            e = host.query_hits_exhaustive(sc, rows, 8, ALL, mask=rm, object_masks=table)
            u = host.query_hits(sc, rows, 8, ALL)
        else:
            w = host.query_sweep(sc, rows, ALL, mask=rm, object_masks=table)
            e = host.query_sweep_exhaustive(sc, rows, ALL, mask=rm, object_masks=table)
            u = host.query_sweep(sc, rows, ALL)
        _CACHE[key] = (sc, rows, table, rm, w, e, u)
    return _CACHE[key]


def no_hidden_object(w, table, rm, what):
    ok = maskset.visible(table, w["object_id"], rm)
    assert ok.all(), (what, "an answer names a hidden object", np.argwhere(~ok)[:6].tolist())


def differs(a, b, names=ALL):
    """Per row: some channel of a and b differs in its bits."""
    out = np.zeros(len(a[names[0]]), bool)
    for k in names:
        out |= ~HC.same(a[k], b[k]).reshape(len(out), -1).all(axis=1)
    return out


# ---- 1. each twin against its exhaustive search, over the visible set ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many_instances", "coincident", "cube"])
def test_nearest_against_the_filtered_exhaustive_search(host, name):
    sc, pts, table, rm, w, e, _ = case(host, "nearest", name)
    dw, de = w["distance"].astype(np.float64), e["distance"].astype(np.float64)
    assert (dw >= de).all(), "the walk is nearer than the exhaustive search over the visible set"
    ni = len(sc.instances)
    worst = 0.0
    for i in np.flatnonzero(w["distance"].view(u32) != e["distance"].view(u32)):
        assert 0 <= e["object_id"][i] < ni, f"row {i}: spheres and planes are never pruned"
        S, W = NC.scale_of(sc, pts[i, :3], int(e["object_id"][i]), int(e["triangle_id"][i]))
        bound = host.nearest_distance_bound(S, W)
        excess = (dw[i] if np.isfinite(dw[i]) else float(pts[i, 3])) - de[i]
        worst = max(worst, excess / bound)
        assert excess <= bound, (name, i, dw[i], de[i], bound)
    no_hidden_object(w, table, rm, name); no_hidden_object(e, table, rm, name + " exhaustive")
    blind = rm == 0
    assert blind.sum() >= 4 and not np.isfinite(w["distance"][blind]).any() and (w["object_id"][blind] == -1).all() and not w["position"][blind].any()
    assert w["stack_max"] <= SC.stack_need(sc)
    print(f"{name}: {len(pts)} rows, {int(np.isfinite(dw).sum())} answered, worst excess / bound {worst:.4f}, stack {w['stack_max']}")


@pytest.mark.parametrize("name", ["many_instances", "coincident", "cube"])
def test_hits_against_the_filtered_exhaustive_search(host, name):
    sc, seg, table, rm, w, e, _ = case(host, "hits", name)
    K = 8
    assert (w["count"] <= e["count"]).all(), "the walk counts more than the visible set holds"
    assert (w["count"][rm == 0] == 0).all() and (e["count"][rm == 0] == 0).all() and np.isinf(w["distance"][rm == 0]).all()
    no_hidden_object(w, table, rm, name); no_hidden_object(e, table, rm, name + " exhaustive")
    found = 0
    for i in range(len(seg)):
        j0, ke = int(min(w["count"][i], K)), int(min(e["count"][i], K))
        keys = [(float(w["distance"][i, j]), int(w["object_id"][i, j]), int(w["triangle_id"][i, j])) for j in range(j0)]
        assert keys == sorted(keys) and np.isinf(w["distance"][i, j0:]).all() and (w["object_id"][i, j0:] == -1).all()
        e_keys = {(int(HC.bits(e["distance"][i, j:j + 1])[0]), int(e["object_id"][i, j]), int(e["triangle_id"][i, j])): j for j in range(ke)}
        for j in range(j0):
            k = (int(HC.bits(w["distance"][i, j:j + 1])[0]), keys[j][1], keys[j][2])
            if k in e_keys:
                for ch in ALL:
                    assert HC.same(w[ch][i, j:j + 1], e[ch][i, e_keys[k]:e_keys[k] + 1]).all(), (name, i, j, ch)
                found += 1
            else:
                last = (float(e["distance"][i, K - 1]), int(e["object_id"][i, K - 1]), int(e["triangle_id"][i, K - 1]))
                assert e["count"][i] > K and keys[j] > last, (name, i, j, "a listed hit the exhaustive search over the visible set does not know")
    assert found > len(seg) // 6
    # the other forms: without a count every listed hit is one of the counted walk's, K = 1 is its head, count-only its count
    one = host.query_hits(sc, seg, 1, ALL, mask=rm, object_masks=table)
    only = host.query_hits(sc, seg, 0, (), mask=rm, object_masks=table)
    assert np.array_equal(only["count"], w["count"]) and np.array_equal(one["count"], w["count"])
    for ch in ALL:
        assert HC.same(one[ch][:, 0], w[ch][:, 0]).all(), ch
    free = host.query_hits(sc, seg, 8, ALL, count=False, mask=rm, object_masks=table)
    no_hidden_object(free, table, rm, name + " without a count")
    assert w["stack_max"] <= SC.stack_need(sc)


@pytest.mark.parametrize("name", ["many_instances", "coincident", "cube"])
def test_sweep_against_the_filtered_exhaustive_search(host, name):
    sc, rows, table, rm, w, e, _ = case(host, "sweep", name)
    tw, te = w["distance"], e["distance"]
    assert (tw >= te).all(), "the walk is earlier than the exhaustive search over the visible set"
    same = tw.view(u32) == te.view(u32)
    assert same.sum() > len(rows) // 2
    for k in ALL:
        a, b = w[k][same], e[k][same]
        if k == "triangle_id":
            SC.same_slots(sc, w["object_id"][same], a, b, name)
            continue
        assert np.array_equal(a.view(u32) if a.dtype == f32 else a, b.view(u32) if b.dtype == f32 else b), (name, k)
    no_hidden_object(w, table, rm, name); no_hidden_object(e, table, rm, name + " exhaustive")
    blind = rm == 0
    assert not np.isfinite(tw[blind]).any() and (w["object_id"][blind] == -1).all() and not w["position"][blind].any()
    assert w["stack_max"] <= SC.stack_need(sc)


@pytest.mark.parametrize("name", ["coincident", "cube"])
def test_sweep_bound_holds_over_the_visible_set(host, name):
    """ACCURACY of rtx_sweep_math.h in fp64, against the scene the row sees: the hidden objects removed."""
    sc, rows, table, rm, w, _, _ = case(host, "sweep", name)
    live = sweepset.is_live(rows)
    checked, worst = 0, 0.0
    for m in np.unique(rm[live]):
        sub, _ = maskset.visible_scene(sc, table, int(m))
        idx = np.flatnonzero(live & (rm == m))[:10]
        if sub is None:
            assert not np.isfinite(w["distance"][idx]).any()
            continue
        for i in idx:
            if np.abs(rows[i, :6]).max() > 1e6:
                continue
            worst = max(worst, SC.check_row(host, sub, rows[i], float(w["distance"][i]), f"{name} row {i} mask {int(m):#x}")); checked += 1
    assert checked >= 24
    print(f"{name}: {checked} rows against fp64 over their visible sets, worst error / bound {worst:.4f}")


# ---- 2. the scene with the hidden objects really removed --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many_instances", "coincident"])
def test_nearest_equals_the_unfiltered_twin_on_the_scene_without_the_hidden_objects(host, name):
    sc, pts, table, rm, w, _, _ = case(host, "nearest", name)
    ni = len(sc.instances)
    checked = 0
    for m in np.unique(rm):
        rows = np.flatnonzero(rm == m)
        sub, ids = maskset.visible_scene(sc, table, int(m))
        if sub is None:
            assert not np.isfinite(w["distance"][rows]).any()
            continue
        assert len(ids) < maskset.object_count(sc) or int(m) == ONES
        s = host.query_nearest(sub, pts[rows], ("distance", "object_id", "triangle_id"))
        for j, i in enumerate(rows):
            da, db = float(w["distance"][i]), float(s["distance"][j])
            if not (np.isfinite(da) or np.isfinite(db)):
                continue
            assert np.isfinite(da) and np.isfinite(db) or np.isfinite(pts[i, 3]), (name, i, da, db)
            obj = int(w["object_id"][i]) if np.isfinite(da) else int(ids[s["object_id"][j]])
            tri = int(w["triangle_id"][i]) if np.isfinite(da) else int(s["triangle_id"][j])
            S, W = NC.scale_of(sc, pts[i, :3], obj, tri) if 0 <= obj < ni else (0.0, 0.0)
            if np.isfinite(db) and 0 <= int(ids[s["object_id"][j]]) < ni:
                S2, W2 = NC.scale_of(sc, pts[i, :3], int(ids[s["object_id"][j]]), int(s["triangle_id"][j]))
                S, W = max(S, S2), max(W, W2)
            bound = host.nearest_distance_bound(S, W)
            a = da if np.isfinite(da) else float(pts[i, 3])
            b = db if np.isfinite(db) else float(pts[i, 3])
            assert abs(a - b) <= bound, (name, i, int(m), da, db, bound)
            checked += 1
    assert checked > len(pts) // 3


# ---- 3. identity forms, mask 0, coincident instances, vacuous passes -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many_instances", "coincident", "chain_blas"])
def test_identity_forms_and_mask_zero(host, name):
    sc = load_scene(name)
    M = maskset.object_count(sc)
    ones_t, zero_t = np.full(M, ONES, u32), np.zeros(M, u32)
    for kind, fn, ex, extra in (("nearest", host.query_nearest, host.query_nearest_exhaustive, ()), ("sweep", host.query_sweep, host.query_sweep_exhaustive, ()),
                                ("hits", host.query_hits, host.query_hits_exhaustive, (8,))):
        rows = np.ascontiguousarray(rows_of(kind, name, sc)[:128])
        n = len(rows)
        names = ALL + (("count",) if kind == "hits" else ())
        plain, plain_ex = fn(sc, rows, *extra, ALL), ex(sc, rows, *extra, ALL)
        forms = {"no table, scalar all ones": dict(mask=ONES), "no table, rows of all ones": dict(mask=np.full(n, ONES, u32)),
                 "a table of all ones": dict(object_masks=ones_t), "a table and rows of all ones, int32": dict(mask=np.full(n, -1, np.int32), object_masks=ones_t.view(np.int32)),
                 "one shared bit": dict(mask=4, object_masks=np.full(M, 0x84, u32))}
        for what, kw in forms.items():
            assert not differs(fn(sc, rows, *extra, ALL, **kw), plain, names).any(), (name, kind, what)
            assert not differs(ex(sc, rows, *extra, ALL, **kw), plain_ex, names).any(), (name, kind, what, "exhaustive")
        assert fn(sc, rows, *extra, ALL, mask=ONES)["stack_max"] == plain["stack_max"]
        for what, kw in {"scalar 0": dict(mask=0), "rows of 0": dict(mask=np.zeros(n, u32), object_masks=ones_t), "a table of 0": dict(mask=ONES, object_masks=zero_t),
                         "no shared bit": dict(mask=3, object_masks=np.full(M, 12, u32))}.items():
            for f in (fn, ex):
                out = f(sc, rows, *extra, ALL, **kw)
                assert np.isinf(out["distance"]).all() and (out["object_id"] == -1).all() and (out["triangle_id"] == -1).all() and (out["material_id"] == -1).all(), (name, kind, what)
                assert not out["position"].any() and not out["normal"].any() and not out["uv"].any()
                assert kind != "hits" or not out["count"].any()
                assert out.get("stack_max", 0) == 0 or what in ("a table of 0", "no shared bit"), "a row whose mask is 0 is not walked"


def test_two_coincident_instances_with_disjoint_masks(host):
    sc = load_scene("coincident")
    table = maskset.coincident_masks(sc)
    pts = np.ascontiguousarray(pointset.generate(sc, 96, seed=3)[0][:160])
    plain = host.query_nearest(sc, pts, ALL)
    both = np.flatnonzero(np.isfinite(plain["distance"]) & (plain["object_id"] == 0))          # the first of the two wins every tie
    assert len(both) >= 16
    first = host.query_nearest(sc, pts, ALL, mask=1, object_masks=table)
    second = host.query_nearest(sc, pts, ALL, mask=2, object_masks=table)
    either = host.query_nearest(sc, pts, ALL, mask=3, object_masks=table)
    assert (first["object_id"][both] == 0).all() and (second["object_id"][both] == 1).all() and (either["object_id"][both] == 0).all()
    for ch in ALL:
        if ch != "object_id":                                                                  # the same mesh in the same place: only the id tells them apart
            assert HC.same(first[ch][both], second[ch][both]).all() and HC.same(first[ch][both], plain[ch][both]).all(), ch
    rm = np.where(np.arange(len(pts)) % 2 == 0, 1, 2).astype(u32)
    mixed = host.query_nearest(sc, pts, ALL, mask=rm, object_masks=table)
    assert np.array_equal(mixed["object_id"][both], np.where(rm[both] == 1, 0, 1))
    # segments through the pair: each instance is listed once per row mask that sees it, twice when the row sees both
    seg = np.ascontiguousarray(hitset.generate(sc, 14, seed=3)[0][:200])
    h = {m: host.query_hits(sc, seg, 8, ALL, mask=m, object_masks=table) for m in (1, 2, 3)}
    pair = lambda out: ((out["object_id"] == 0) | (out["object_id"] == 1)).sum(axis=1)
    assert (h[1]["object_id"] != 1).all() and (h[2]["object_id"] != 0).all() and pair(h[1]).sum() > 20
    short = h[3]["count"] <= 8                                                                 # nothing cut off the list
    assert np.array_equal(h[1]["count"], h[2]["count"]) and short.sum() > len(seg) // 2 and np.array_equal(pair(h[3])[short], 2 * pair(h[1])[short])
    assert np.array_equal((h[3]["count"] - h[1]["count"])[short], pair(h[1])[short])
    sw = {m: host.query_sweep(sc, np.ascontiguousarray(sweepset.generate(sc, 96, seed=3)[0][:160]), ALL, mask=m, object_masks=table) for m in (1, 2)}
    hit0 = sw[1]["object_id"] == 0
    assert hit0.sum() >= 16 and (sw[2]["object_id"][hit0] == 1).all() and HC.same(sw[1]["distance"], sw[2]["distance"]).all()


@pytest.mark.parametrize("kind", ["nearest", "hits", "sweep"])
@pytest.mark.parametrize("name", ["many_instances", "coincident", "cube"])
def test_the_filter_changes_some_rows_and_not_others(host, kind, name):
    _, rows, _, rm, w, _, u = case(host, kind, name)
    names = ALL + (("count",) if kind == "hits" else ())
    changed = differs(w, u, names)
    assert changed.sum() >= 8 and (~changed & (rm != 0) & np.isfinite(np.asarray(u["distance"]).reshape(len(rows), -1)[:, 0])).sum() >= 8, (kind, name, int(changed.sum()))


# ---- 4. the stand-alone check, declarations, the Python layer -------------------------------------------------------------------------------------
def test_mask_check_program():
    """csrc/mask_check.cpp: the three filtered walks against the filtered exhaustive searches on generated trees, under the host sanitizers."""
    out = subprocess.run(["make", "-B", "-C", os.path.join(REPO, "cpu-raytracer_amd", "csrc"), "mask_check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "mask_check: ok" in out.stdout
    assert re.search(r"deepest stack \d+ of 64", out.stdout)


def test_functions_are_declared_exported_and_bound(host):
    from pyrtx import api
    header = open(os.path.join(REPO, "include", "rtx.h")).read()
    for name in api.MASK_EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in api.EXPORTS and name in api.OPTIONAL_EXPORTS
    assert re.search(r"typedef struct rtx_query_filter \{\s*const uint32_t \* row_masks_dev;[^}]*uint32_t row_mask;\s*\} rtx_query_filter;", header)
    lib = api.load_library()
    for name in api.MASK_EXPORTS:
        assert getattr(lib, name).restype is api.C.c_int
    host_header = open(os.path.join(REPO, "include", "rtx_host.h")).read()
    for q in ("nearest", "hits", "sweep"):
        for form in ("", "_exhaustive"):
            assert re.search(r"\bint\s+rtxh_query_%s%s_filtered\s*\(" % (q, form), host_header)


def test_python_checks_come_before_the_library(host):
    sc = load_scene("coincident")
    pts = np.zeros((4, 4), f32); pts[:, 3] = 1
    M = maskset.object_count(sc)
    with pytest.raises(TypeError):
        host.query_nearest(sc, pts, mask=np.zeros(4, np.float32))
    with pytest.raises(TypeError):
        host.query_nearest(sc, pts, object_masks=np.zeros(M, np.int64))
    with pytest.raises(ValueError):
        host.query_nearest(sc, pts, mask=np.zeros(5, u32))
    with pytest.raises(ValueError):
        host.query_nearest(sc, pts, object_masks=np.zeros(M + 1, u32))
    with pytest.raises(ValueError):
        host.query_hits(sc, np.zeros((4, 7), f32), mask=1 << 32)
    assert np.array_equal(maskset.visible(np.array([1, 2, 0], u32), np.array([[0, 1, 2, -1]] * 2), np.array([1, 3], u32)),
                          [[True, False, False, True], [True, True, False, True]])
