"""The filtered walk queries on the GPU (query_nearest / query_hits / query_sweep with mask=..., set_object_masks: rtx_query_*_filtered and the
object-mask table).  Every comparison is bit for bit (NaN == NaN) against the host twin (host.query_* with mask= and object_masks=, the same
code of csrc/rtx_*_math.h) run on the arrays AND the masks read back from the context:
  * many_instances (160 instances, a sphere, a plane) under seeded random 4-bit object masks, with the sphere and the plane hidden in one
    variant; coincident, whose two coincident instances get different masks; chain_blas, whose visible rows reach the spill region;
  * rows of pointset.py, hitset.py (K in {1, 8} with a count, K = 8 without, count only) and sweepset.py, at most 448 of them, with per-row
    masks from {0, one bit, two bits, all ones} and rows of mask 0 on both sides of every wave boundary;
  * in every scene some row's answer differs from the unfiltered one and some row's does not; no answer names a hidden object;
  * the identity forms (mask=None, a NULL filter through the raw entry point, no table with 0xFFFFFFFF, all ones everywhere) equal today's call;
  * sort=True against unsorted with per-row masks; batches of 257 and 65 rows; guard elements; RTX_QUERY_GRID=1;
  * the table set from numpy and from a device tensor, read back, changed between two calls without a wait, kept across update_instances, dropped;
  * the errors in their documented order; K = 1 against query_closest and the count against query_occluded."""
import copy
import ctypes as C

import numpy as np
import pytest

import hitset
import maskset
import test_gpu_query_hits as H
import test_gpu_query_nearest as N
import test_gpu_query_sweep as S
import test_gpu_query_tiles as T
from test_gpu_query import check_channels, dev, host as to_host, same_bits
from test_gpu_query_hits import check

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
ALL = hitset.ALL
ONES = maskset.ALL_ONES
INVALID, STATE = 1, 5
LDS_STACK = 16                                                              # RTX_LDS_STACK
KINDS = ("nearest", "hits", "sweep")
SCENES = ("many_instances", "coincident", "chain_blas")
# scene -> (seed of the object masks, seed of the row masks), chosen on the CPU with the host twin (tests/test_query_masks_cpu.py runs the same
# generators) so that the filter changes some rows and leaves others as they were
SEEDS = {"many_instances": (3, 7), "coincident": (0, 5), "chain_blas": (0, 9)}
FORMS = {"nearest": {"all channels": {}}, "sweep": {"all channels": {}},
         "hits": {"K 8 with count": dict(max_hits=8, channels=ALL), "K 8 no count": dict(max_hits=8, channels=ALL, count=False),
                  "K 1 with count": dict(max_hits=1, channels=ALL), "count only": dict(max_hits=0, channels=())}}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def rows_of(kind, name):
    """(scene, rows (<= 448), labels): the rows of the kind's own GPU test."""
    sc, rows, labels, _ = {"nearest": N, "hits": H, "sweep": S}[kind].generated(name)
    assert len(rows) <= 448
    return sc, rows, labels


def more_rows(kind, name):
    """(scene, more than a tile of rows, at most 448): rows_of, and the same generator at another seed behind them."""
    sc, rows, _ = rows_of(kind, name)
    again = {"nearest": lambda: N.generated(name, seed=35), "hits": lambda: H.generated(name, seed=9), "sweep": lambda: S.generated(name, seed=35)}[kind]()[1]
    rows = np.ascontiguousarray(np.concatenate([rows, again])[:448])
    assert len(rows) > 256
    return sc, rows


def table_of(name, sc, hide_world=False):
    if name == "coincident":
        return maskset.coincident_masks(sc)
    if name == "chain_blas":
        return np.array([5], u32)                                           # one instance, seen by bits 0 and 2
    return maskset.object_masks(sc, SEEDS[name][0], hide_world)


def as_tensor(masks):
    """uint32 masks as the int32 device tensor the API takes (torch has no general uint32): the same bits."""
    return dev(np.ascontiguousarray(masks, u32).view(np.int32))


def device(r, kind, rows_t, mask, sort=False, n=None, out=None):
    """Every form of the kind's call -> {form: tensors}."""
    fn = {"nearest": r.query_nearest, "hits": r.query_hits, "sweep": r.query_sweep}[kind]
    if kind == "hits":
        return {form: fn(rows_t, kw["max_hits"], kw["channels"], count=kw.get("count", True), n=n, sort=sort, mask=mask) for form, kw in FORMS[kind].items()}
    return {"all channels": fn(rows_t, ALL, n=n, sort=sort, mask=mask, out=out)}


def twin(kind, state, blas, rows, mask, table):
    """The host twin on the arrays read back, the same forms; "stack_max" of the first form kept aside under the key None."""
    from pyrtx import host
    fn = {"nearest": host.query_nearest, "hits": host.query_hits, "sweep": host.query_sweep}[kind]
    out = {}
    for form, kw in FORMS[kind].items():
        if kind == "hits":
            o = fn(state, rows, kw["max_hits"], kw["channels"], kw.get("count", True), blas=blas, mask=mask, object_masks=table)
        else:
            o = fn(state, rows, ALL, blas=blas, mask=mask, object_masks=table)
        out.setdefault(None, o.pop("stack_max"))
        out[form] = o
    return out


def compare(kind, got, want, labels, what):
    for form, o in got.items():
        assert tuple(o) == tuple(want[form]), (what, form, tuple(o), tuple(want[form]))
        (check if kind == "hits" else check_channels)(o, want[form], labels, f"{what}, {form}")


def rows_that_differ(a, b):
    """Per row: some array of form-dicts a and b differs in its bits."""
    out = None
    for form in a:
        for k in a[form]:
            x, y = (to_host(t) if hasattr(t, "cpu") else t for t in (a[form][k], b[form][k]))
            d = ~same_bits(x, y)
            out = d if out is None else out | d
    return out


def no_hidden_object(got, table, rm, what):
    for form, o in got.items():
        if "object_id" in o:
            ids = to_host(o["object_id"])
            ok = maskset.visible(table, ids, rm[:len(ids)])
            assert ok.all(), (what, form, "an answer names a hidden object", np.argwhere(~ok)[:6].tolist())


# ---- 1. parity with the host twin, per-row masks, sorted and unsorted ------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("kind", KINDS)
def test_device_equals_the_filtered_host_walk(api, kind, name):
    sc, rows, labels = rows_of(kind, name)
    table, rm = table_of(name, sc), maskset.row_masks(len(rows), SEEDS[name][1])
    assert (rm[63:65] == 0).all() and (rm != 0).sum() > len(rows) // 2
    r = api.Renderer(sc)
    r.set_object_masks(table)
    back = r.read_object_masks()
    assert back.dtype == u32 and np.array_equal(back, table)
    state, blas = N.read_back(r, sc)
    want = twin(kind, state, blas, rows, rm, back)
    if name == "chain_blas" and kind != "hits":                             # the chain is walked end to end by points and by balls
        assert want[None] > LDS_STACK, "the visible rows of this scene are here to reach the spill region"
    rows_t, rm_t = dev(rows), as_tensor(rm)
    got = device(r, kind, rows_t, rm_t)
    compare(kind, got, want, labels, f"{kind} {name}")
    compare(kind, device(r, kind, rows_t, rm_t, sort=True), want, labels, f"{kind} {name} sorted")
    no_hidden_object(got, back, rm, f"{kind} {name}")
    # against vacuous passes: the filter changed some rows and left others, which see something, as they were
    plain = device(r, kind, rows_t, None)
    changed = rows_that_differ(got, plain)
    first = to_host(next(iter(plain.values())).get("distance", next(iter(plain.values())).get("count"))).reshape(len(rows), -1)[:, 0]
    assert changed.sum() >= 8 and (~changed & (rm != 0) & np.isfinite(first)).sum() >= 8, (kind, name, int(changed.sum()))
    # rows of mask 0: the no-answer values, count 0
    blind = rm == 0
    for form, o in got.items():
        if "distance" in o:
            assert np.isinf(to_host(o["distance"])[blind]).all() and (to_host(o["object_id"])[blind] == -1).all() and not to_host(o["position"])[blind].any(), form
        if "count" in o:
            assert not to_host(o["count"])[blind].any(), form
    if name == "coincident":                                                # the visible one of the coincident pair is reported, and it changes with the row mask
        by_mask = {m: device(r, kind, rows_t, m) for m in (1, 2)}
        compare(kind, by_mask[1], twin(kind, state, blas, rows, 1, back), labels, f"{kind} coincident mask 1")
        compare(kind, by_mask[2], twin(kind, state, blas, rows, 2, back), labels, f"{kind} coincident mask 2")
        form = next(iter(by_mask[1]))
        a, b = to_host(by_mask[1][form]["object_id"]), to_host(by_mask[2][form]["object_id"])
        assert (a != 1).all() and (b != 0).all() and (a == 0).sum() >= 8 and np.array_equal(a == 0, b == 1)


@pytest.mark.parametrize("kind", KINDS)
def test_the_sphere_and_the_plane_hidden_and_a_scalar_mask(api, kind):
    """The table comes from a device tensor here; the rows share one mask."""
    sc, rows, labels = rows_of(kind, "many_instances")
    table = table_of("many_instances", sc, hide_world=True)
    ni = len(sc.instances)
    assert len(table) == ni + 2 and not table[ni:].any()
    r = api.Renderer(sc)
    r.set_object_masks(as_tensor(table))
    back = r.read_object_masks()
    assert np.array_equal(back, table)
    state, blas = N.read_back(r, sc)
    rows_t = dev(rows)
    plain = device(r, kind, rows_t, None)
    form = next(iter(plain))
    assert (to_host(plain[form]["object_id"]) >= ni).any(), "the sphere or the plane answers some row when nothing is hidden"
    for m in (2, 0x80000000 | 4, ONES):
        got = device(r, kind, rows_t, m)
        compare(kind, got, twin(kind, state, blas, rows, m, back), labels, f"{kind} world hidden, mask {m:#x}")
        no_hidden_object(got, back, np.full(len(rows), m, u32), f"{kind} mask {m:#x}")
        assert (to_host(got[form]["object_id"]) < ni).all()


# ---- 2. the identity forms -----------------------------------------------------------------------------------------------------------------------
def raw_call(api, r, kind, rows_t, n, filt, out, K=8):
    """The C entry point with the filter pointer given as it is (None: NULL), on the context's stream."""
    import torch
    buf = api.RtxQueryBuffers()
    for name in ALL:
        setattr(buf, name, out[name].data_ptr())
    torch.cuda.synchronize()
    f = None if filt is None else C.byref(filt)
    if kind == "hits":
        rc = r.lib.rtx_query_hits_filtered(r.ctx, rows_t.data_ptr(), n, K, api.RTX_QUERY_ALL, C.byref(buf), out["count"].data_ptr(), 0, f)
    else:
        rc = getattr(r.lib, f"rtx_query_{kind}_filtered")(r.ctx, rows_t.data_ptr(), n, api.RTX_QUERY_ALL, C.byref(buf), 0, f)
    r.synchronize()
    return rc


@pytest.mark.parametrize("kind", KINDS)
def test_identity_forms_equal_the_unfiltered_call(api, kind):
    sc, rows, labels = rows_of(kind, "many_instances")
    n = len(rows)
    r = api.Renderer(sc)
    rows_t = dev(rows)
    today = {form: {k: to_host(t) for k, t in o.items()} for form, o in device(r, kind, rows_t, None).items()}
    state, blas = N.read_back(r, sc)
    compare(kind, today, twin(kind, state, blas, rows, None, None), labels, f"{kind} mask=None")
    assert r.read_object_masks() is None
    compare(kind, device(r, kind, rows_t, ONES), today, labels, f"{kind} no table, scalar all ones")
    compare(kind, device(r, kind, rows_t, -1), today, labels, f"{kind} no table, scalar -1")
    first = next(iter(today))
    for filt, what in ((None, "a NULL filter"), (api.RtxQueryFilter(None, ONES), "a filter of all ones")):
        out = T.out_tensors(api, n, 8 if kind == "hits" else 0, kind == "hits")
        assert raw_call(api, r, kind, rows_t, n, filt, out) == 0
        (check if kind == "hits" else check_channels)(out, today[first], labels, f"{kind} raw entry point, {what}")
    r.set_object_masks(np.full(maskset.object_count(sc), ONES, u32))
    compare(kind, device(r, kind, rows_t, as_tensor(np.full(n, ONES, u32))), today, labels, f"{kind} a table of all ones, rows of all ones")
    compare(kind, device(r, kind, rows_t, None), today, labels, f"{kind} a table set, mask=None")
    r.set_object_masks(np.full(maskset.object_count(sc), 0x40, np.int32))
    compare(kind, device(r, kind, rows_t, 0x40), today, labels, f"{kind} one shared bit")
    none = device(r, kind, rows_t, 0x3f)                                     # no shared bit: walked, and nothing is seen
    for form, o in none.items():
        assert "distance" not in o or np.isinf(to_host(o["distance"])).all()
        assert "count" not in o or not to_host(o["count"]).any()


# ---- 3. batch sizes, guards, tiles -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_batches_of_257_and_65_rows(api, kind):
    name = "many_instances" if kind != "hits" else "coincident"
    sc, rows = more_rows(kind, name)
    labels = None
    table, rm = table_of(name, sc), maskset.row_masks(len(rows), 23)
    r = api.Renderer(sc)
    r.set_object_masks(table)
    state, blas = N.read_back(r, sc)
    want = twin(kind, state, blas, rows, rm, r.read_object_masks())
    rows_t = dev(rows)
    for n in (257, 65):
        rm_t = as_tensor(rm[:n])
        for sort in (False, True):
            got = device(r, kind, rows_t, rm_t, sort=sort, n=n)
            assert all(len(t) == n for o in got.values() for t in o.values())
            compare(kind, got, want, labels, f"{kind} n {n} sort {sort}")


@pytest.mark.parametrize("kind", KINDS)
def test_guard_elements_stay_untouched(api, kind):
    import torch
    sc, rows, labels = rows_of(kind, "coincident")
    n, pad = min(len(rows), 200) - 3, 64
    table, rm = table_of("coincident", sc), maskset.row_masks(n, 29)
    r = api.Renderer(sc)
    r.set_object_masks(table)
    state, blas = N.read_back(r, sc)
    want = twin(kind, state, blas, rows[:n], rm, table)
    K = 8 if kind == "hits" else 0
    big = T.out_tensors(api, n + pad, K, kind == "hits")
    masks = torch.full((pad + n + pad,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")      # the row masks between neighbours that would show up as masks
    masks[pad:pad + n] = as_tensor(rm)
    rows_t = dev(rows)
    for sort in (False, True):
        out = {k: t[:n] for k, t in big.items()}
        fn = {"nearest": r.query_nearest, "hits": r.query_hits, "sweep": r.query_sweep}[kind]
        got = fn(rows_t, 8, ALL, out=out, n=n, sort=sort, mask=masks[pad:pad + n]) if kind == "hits" else fn(rows_t, ALL, out=out, n=n, sort=sort, mask=masks[pad:pad + n])
        (check if kind == "hits" else check_channels)(got, want["K 8 with count" if kind == "hits" else "all channels"], labels, f"{kind} guards sort {sort}")
        for k, t in big.items():
            assert (t[n:] == -77).all(), (kind, k, sort, "elements after row n - 1 were written")
        assert (masks[:pad] == 0x5a5a5a5a).all() and (masks[pad + n:] == 0x5a5a5a5a).all() and torch.equal(masks[pad:pad + n], as_tensor(rm))


@pytest.mark.parametrize("name", ["many_instances", "chain_blas"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_workgroup_walks_several_tiles(api, monkeypatch, kind, name):
    """RTX_QUERY_GRID=1: the second tile's lanes carry nothing of the first tile's masks, either way round."""
    sc, rows = more_rows(kind, name)
    labels = None
    table = table_of(name, sc)
    rm = maskset.row_masks(len(rows), 31)
    flipped = np.where(np.arange(len(rows)) < T.TILE, np.roll(rm, 7), rm).astype(u32)
    flipped[:T.TILE][::3] = 0                                               # many blind lanes in the first tile, whose slots see again in the second
    r = T.renderer(api, monkeypatch, sc, grid=1)
    r.set_object_masks(table)
    state, blas = N.read_back(r, sc)
    rows_t = dev(rows)
    for masks in (rm, flipped):
        want = twin(kind, state, blas, rows, masks, table)
        for sort in (False, True):
            compare(kind, device(r, kind, rows_t, as_tensor(masks), sort=sort), want, labels, f"{kind} {name} grid 1 sort {sort}")


# ---- 4. the table -----------------------------------------------------------------------------------------------------------------------------------
def test_the_table_set_read_changed_kept_and_dropped(api):
    sc, rows, labels = rows_of("nearest", "many_instances")
    M = maskset.object_count(sc)
    t1, t2 = maskset.object_masks(sc, 3), maskset.object_masks(sc, 4)
    rm = maskset.row_masks(len(rows), 7)
    r = api.Renderer(sc)
    assert r.read_object_masks() is None
    state, blas = N.read_back(r, sc)
    rows_t, rm_t = dev(rows), as_tensor(rm)
    want = {k: twin("nearest", state, blas, rows, rm, t) for k, t in (("t1", t1), ("t2", t2), ("none", None))}
    assert rows_that_differ({"a": want["t1"]["all channels"]}, {"a": want["t2"]["all channels"]}).sum() >= 8
    # set from numpy (uint32 and int32: the same bits), from a device tensor, read back
    r.set_object_masks(t1)
    assert np.array_equal(r.read_object_masks(), t1)
    r.set_object_masks((t1 | u32(0x80000000)).view(np.int32))
    assert np.array_equal(r.read_object_masks(), t1 | u32(0x80000000))
    r.set_object_masks(as_tensor(t2))
    assert np.array_equal(r.read_object_masks(), t2)
    # changed between two calls on the stream without a wait: each call sees the table of its moment
    r.set_object_masks(t1)
    a = r.query_nearest(rows_t, ALL, mask=rm_t)
    r.set_object_masks(t2)
    b = r.query_nearest(rows_t, ALL, mask=rm_t)
    r.set_object_masks(as_tensor(t1))
    c = r.query_nearest(rows_t, ALL, mask=rm_t)
    r.set_object_masks(None)
    d = r.query_nearest(rows_t, ALL, mask=rm_t)
    check_channels(a, want["t1"]["all channels"], labels, "first table")
    check_channels(b, want["t2"]["all channels"], labels, "second table, set from the host")
    check_channels(c, want["t1"]["all channels"], labels, "first table again, set from the device")
    check_channels(d, want["none"]["all channels"], labels, "dropped")
    assert r.read_object_masks() is None
    # kept across update_instances: the TLAS is rebuilt, the table is the one that was set
    r.set_object_masks(t2)
    pos = np.ascontiguousarray(sc.instances["world"][:, [3, 7, 11]], f32)
    rot = np.tile(np.array([0, 0, 0, 1], f32), (len(pos), 1))
    p_t, q_t = dev(pos), dev(rot)
    r.update_instances(p_t, q_t)
    assert np.array_equal(r.read_object_masks(), t2)
    moved, blas = N.read_back(r, sc)
    check_channels(r.query_nearest(rows_t, ALL, mask=rm_t), twin("nearest", moved, blas, rows, rm, t2)["all channels"], labels, "after update_instances")
    r.set_frame(sc)                                                          # the same counts: the table stays
    assert np.array_equal(r.read_object_masks(), t2)
    check_channels(r.query_nearest(rows_t, ALL, mask=rm_t), want["t2"]["all channels"], labels, "after set_frame")
    assert M == len(t2)


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_in_their_documented_order(api):
    import torch
    sc, rows, labels = rows_of("nearest", "coincident")
    M = maskset.object_count(sc)
    table = maskset.coincident_masks(sc)
    n = len(rows)
    r = api.Renderer(sc)
    lib = r.lib
    cnt = C.c_int32(-5)
    keep = np.zeros(M + 1, u32)
    d_masks = as_tensor(keep)
    torch.cuda.synchronize()
    # a wrong count, a NULL pointer with a count, a NULL context
    for fn, ptr in ((lib.rtx_set_object_masks, keep.ctypes.data), (lib.rtx_update_object_masks, d_masks.data_ptr())):
        assert fn(r.ctx, ptr, M + 1) == INVALID and fn(r.ctx, ptr, M - 1) == INVALID and fn(r.ctx, ptr, 0) == INVALID and fn(r.ctx, None, M) == INVALID
        assert fn(None, ptr, M) == INVALID
        assert fn(r.ctx, None, 0) == 0 and fn(r.ctx, ptr, M) == 0
    assert lib.rtx_read_object_masks(r.ctx, None, 0, None) == INVALID and lib.rtx_read_object_masks(r.ctx, keep.ctypes.data, M - 1, C.byref(cnt)) == INVALID and cnt.value == M
    assert lib.rtx_read_object_masks(r.ctx, keep.ctypes.data, -1, C.byref(cnt)) == INVALID
    assert lib.rtx_read_object_masks(r.ctx, None, 0, C.byref(cnt)) == 0 and cnt.value == M
    with pytest.raises(api.RtxError) as e:
        r.set_object_masks(np.zeros(M + 2, u32))
    assert e.value.code == INVALID
    # before rtx_set_frame
    empty = api.Renderer(sc, upload=False)
    assert lib.rtx_set_object_masks(empty.ctx, keep.ctypes.data, M) == STATE and lib.rtx_update_object_masks(empty.ctx, d_masks.data_ptr(), M) == STATE
    assert lib.rtx_set_object_masks(empty.ctx, None, 0) == STATE and lib.rtx_read_object_masks(empty.ctx, None, 0, C.byref(cnt)) == STATE
    # the filtered calls: the errors of the unfiltered call first, in its order
    rows_t = dev(rows)
    dist = torch.full((n,), -77.0, dtype=torch.float32, device="cuda")
    count = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    buf = api.RtxQueryBuffers(); buf.distance = dist.data_ptr()
    filt = api.RtxQueryFilter(None, 1)
    torch.cuda.synchronize()
    pp, D, B, F = rows_t.data_ptr(), api.RTX_QUERY_DISTANCE, C.byref(buf), C.byref(filt)
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, 0, D, B, 0, F) == INVALID and lib.rtx_query_nearest_filtered(r.ctx, pp, n, 0, B, 0, F) == INVALID
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, n, D, B, 1, F) == INVALID and lib.rtx_query_nearest_filtered(None, pp, n, D, B, 0, F) == INVALID
    assert lib.rtx_query_nearest_filtered(empty.ctx, pp, n, D, B, 0, F) == STATE and lib.rtx_query_nearest_filtered(empty.ctx, pp, n, 0, B, 0, F) == INVALID
    # a frame with other counts after the table was set: RTX_ERR_STATE, nothing queued, the outputs untouched; the unfiltered calls go on
    r.set_object_masks(table)
    other = copy.copy(sc)
    other.planes = sc.planes[:0].copy()
    assert len(sc.planes) == 1
    r.set_frame(other)
    assert np.array_equal(r.read_object_masks(), table), "rtx_set_frame keeps the table"
    seg_t = dev(H.generated("coincident")[1][:n]); sw_t = dev(S.generated("coincident")[1][:n])
    m = min(n, len(seg_t), len(sw_t))
    torch.cuda.synchronize()
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, n, D, B, 0, F) == STATE
    assert b"object masks" in lib.rtx_last_error(r.ctx)
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, n, 0, B, 0, F) == INVALID, "the argument checks come first"
    assert lib.rtx_query_hits_filtered(r.ctx, seg_t.data_ptr(), m, 1, D, B, count.data_ptr(), 0, F) == STATE
    assert lib.rtx_query_hits_filtered(r.ctx, seg_t.data_ptr(), m, 0, 0, None, count.data_ptr(), 0, F) == STATE
    assert lib.rtx_query_sweep_filtered(r.ctx, sw_t.data_ptr(), m, D, B, 0, F) == STATE
    r.synchronize()
    assert (dist == -77.0).all() and (count == -77).all()
    with pytest.raises(api.RtxError) as e:
        r.query_nearest(rows_t, "distance", mask=1)
    assert e.value.code == STATE
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, n, D, B, 0, None) == 0, "a NULL filter is the unfiltered call"
    assert lib.rtx_set_object_masks(r.ctx, keep.ctypes.data, M) == INVALID and lib.rtx_set_object_masks(r.ctx, keep.ctypes.data, M - 1) == 0      # M of the CURRENT frame
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, n, D, B, 0, F) == 0
    r.set_object_masks(None)
    r.set_frame(sc)
    assert lib.rtx_query_nearest_filtered(r.ctx, pp, n, D, B, 0, F) == 0
    r.synchronize()
    from pyrtx import host
    state, blas = N.read_back(r, sc)
    assert same_bits(to_host(dist), host.query_nearest(state, rows, "distance", blas=blas, mask=1)["distance"]).all()
    # the Python layer checks before the library is reached
    with pytest.raises(TypeError):
        r.query_nearest(rows_t, "distance", mask=dev(np.zeros(n, f32)))
    with pytest.raises(ValueError):
        r.query_nearest(rows_t, "distance", mask=as_tensor(np.zeros(n + 1, u32)))
    with pytest.raises(ValueError):
        r.query_nearest(rows_t, "distance", mask=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError):
        r.query_nearest(rows_t, "distance", mask=np.zeros(n, u32))
    with pytest.raises(TypeError):
        r.set_object_masks(np.zeros(M, np.int64))
    with pytest.raises(ValueError):
        r.query_sweep(sw_t, "distance", mask=1 << 32)


# ---- 6. consistency with the unfiltered production path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_k1_against_query_closest_and_the_count_against_query_occluded(api, name):
    sc, seg, labels = rows_of("hits", name)
    r = api.Renderer(sc)
    far = seg.copy(); far[:, 6] = np.inf
    one = {k: to_host(t) for k, t in r.query_hits(dev(far), 1, ALL, mask=ONES).items()}
    closest = {k: to_host(t) for k, t in r.query_closest(dev(np.ascontiguousarray(far[:, :6])), ALL).items()}
    cd = closest["distance"]
    assert not np.isnan(cd).any() and (one["distance"][:, 0] <= cd).all()                       # a miss is +inf on both sides
    head = np.flatnonzero(np.isfinite(cd) & (one["distance"][:, 0].view(u32) == cd.view(u32)) & (one["object_id"][:, 0] == closest["object_id"])
                          & (one["triangle_id"][:, 0] == closest["triangle_id"]))
    assert len(head) > len(seg) // 4, (name, len(head), int(np.isfinite(cd).sum()))      # where the head IS the closest hit every channel is query_closest's
    for ch in ALL:
        assert same_bits(one[ch][head, 0], closest[ch][head]).all(), (name, ch)
    if len(sc.spheres) == 0:                                                 # the rule of the hits tests: Sphere::intersect is other arithmetic
        count = to_host(r.query_hits(dev(seg), 0, (), mask=ONES)["count"])
        occ = to_host(r.query_occluded(dev(seg)))
        assert np.array_equal(occ != 0, count > 0), (name, np.flatnonzero((occ != 0) != (count > 0))[:8])
        assert 10 < (count > 0).sum() < len(seg) - 10


def test_two_scenes_without_spheres_are_checked_against_query_occluded():
    assert sum(len(H.load_scene(n).spheres) == 0 for n in SCENES) >= 2
