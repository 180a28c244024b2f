"""rtx_blas_pseudonormals / rtx_query_signed_distance on the GPU.  Everything is compared bit for bit (NaN == NaN) against the host twins
(rtxh_blas_pseudonormals, rtxh_query_signed_distance: csrc/rtx_side_math.h compiled for the CPU, tests/test_query_signed_cpu.py) on arrays read
back from the context; the only other reference is the float64 winding number of the sign-oracle test, under the leave-out rule and the cap of
the CPU test.

  tables   read_blas_pseudonormals == host.blas_pseudonormals: 1 triangle, 85 / 86 triangles, 255 / 256 / 257 vertices, fans of valence 65 and
           257, Rock, Torus, Monkey, an SBVH tree whose slot table repeats triangles, hostile positions, a positions tensor 4 bytes into its
           allocation; after build_blas with the slots of that build (pad triangles included), after refit_blas;
  query    signed_distance, feature and every channel at n = 1 ... 1000, one workgroup walking tile after tile (RTX_QUERY_GRID=1), sorted,
           masks as an int and as a tensor, the chain scene (spill region), a frame mixing a mesh with tables, one without (+ 8), spheres and
           planes, after update_instances, a guard word behind every output, channel subsets, the channels of query_nearest;
  oracle   300 rows around posed Rock and Torus against the numpy winding number;
  state    alloc_blas, rtx_upload_blas and rtx_alloc_blas_topology over the id drop the tables (+ 8 afterwards); every error code in order —
           the argument errors, then RTX_ERR_STATE / RTX_ERR_LIMIT as for rtx_query_nearest, then the state rule of the filtered queries —
           and a valid query after them; the calls queued between frames without a wait.
"""
import ctypes as C

import numpy as np
import pytest

import normalset as ns
import sideset as ss
import util
from test_gpu_query import check_channels, same_bits
from test_gpu_rays import chain_blas_scene

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
INVALID, LIMIT, STATE = 1, 4, 5
PATTERN = 0x5ca1ab1e
ALL = ("distance", "position", "normal", "uv", "material_id", "object_id", "triangle_id")
IDENTITY = (np.zeros((1, 3), f32), np.array([[0, 0, 0, 1]], f32))


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def dev(a, dtype=f32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def make_tables(r, meshes, ids=None, positions=None):
    """bind + topology + pseudonormals for the BLAS ids (all), from the meshes' own positions or positions[b] -> the tensors to keep alive."""
    import torch
    keep = []
    for b in (range(len(meshes)) if ids is None else ids):
        pos, idx, _, sv = meshes[b]
        p = dev(pos if positions is None else positions[b]); i = dev(idx, np.int32)
        keep += [p, i]
        torch.cuda.synchronize()
        r.bind_blas_vertices(b, sv, len(pos))
        r.set_blas_topology(b, i, len(pos))
        r.blas_pseudonormals(b, p)
    return keep


def read_back(r, sc):
    inst, nodes, idx = r.read_frame_state()
    return (inst, nodes, idx, sc.spheres, sc.planes), [r.read_blas(b) for b in range(len(sc.blas))]


def twin(r, sc, meshes, rows, ids, channels=ALL, **kw):
    """The host twin over what the context holds now: frame state, BLAS arrays and pseudonormal tables all read back."""
    from pyrtx import host
    arrays, blas = read_back(r, sc)
    tables = {b: r.read_blas_pseudonormals(b) + (meshes[b][3],) for b in ids}
    return host.query_signed_distance(arrays, rows, channels, blas=blas, pseudonormals=tables, **kw)


def guarded(n, k, dtype):
    """A device tensor of shape (n,) / (n, k) in an allocation with PATTERN words behind it -> (tensor, guard)"""
    import torch
    whole = torch.full((n * k + 4,), PATTERN, dtype=torch.int32, device="cuda")
    t = whole[:n * k].view(torch.float32 if dtype == np.float32 else torch.int32)
    return (t.view(n, k) if k > 1 else t), whole[n * k:]


def signed_query(api, r, rows_t, channels=ALL, n=None, **kw):
    """query_signed_distance into guarded outputs -> {name: numpy}, after checking every guard."""
    import torch
    n = int(rows_t.shape[0]) if n is None else n
    names = api.query_names(channels) if len(channels) else ()
    out, guards = {}, []
    for name in names:
        _, dt, k = api.QUERY_CHANNELS[name]
        out[name], g = guarded(n, k, dt); guards.append((name, g))
    out["signed_distance"], g = guarded(n, 1, np.float32); guards.append(("signed_distance", g))
    if kw.get("feature", True):
        out["feature"], g = guarded(n, 1, np.int32); guards.append(("feature", g))
    torch.cuda.synchronize()
    got = r.query_signed_distance(rows_t, channels, out=out, n=n, **{"feature": True, **kw})
    r.synchronize()
    for name, g in guards:
        assert bool((g == PATTERN).all()), f"memory behind {name} was written"
    return {k: v.cpu().numpy() for k, v in got.items()}


def mixed_rows(n, seed, box=5.0, rmax=6.0):
    rng = np.random.default_rng(seed)
    rows = ss.as_rows(rng.uniform(-box, box, (n, 3)), rmax)
    if n >= 8:
        rows[3] = (np.nan, 0, 0, 1); rows[5, 3] = 0.0; rows[6, 3] = -1.0; rows[7] = (50, 50, 50, 0.5)
    return rows


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
def table_cases():
    cases = {k: v for k, v in ns.shapes().items() if k != "V1"}
    for m in ("Rock", "Torus", "Monkey"):
        cases[m] = ns.indexed(m)
    return cases


TABLE_CASES = table_cases()


def one_mesh_renderer(api, pos, idx, **kw):
    meshes = [(pos, idx) + ss.mesh_blas(pos, idx, **kw)]
    sc = ss.posed_scene(meshes, *IDENTITY)
    return api.Renderer(sc), sc, meshes


@pytest.mark.parametrize("name", list(TABLE_CASES) + ["Monkey_sbvh"])
def test_tables_parity_with_the_host_twin(api, name):
    from pyrtx import host
    pos, idx = TABLE_CASES["Monkey" if name == "Monkey_sbvh" else name]
    r, sc, meshes = one_mesh_renderer(api, pos, idx, **({"reference_sbvh": True} if name == "Monkey_sbvh" else {}))
    sv = meshes[0][3]
    if name == "Monkey_sbvh":
        assert len(sv) > len(idx), "the slot table repeats triangles"
    keep = make_tables(r, meshes)
    vert, edge = r.read_blas_pseudonormals(0)
    want_v, want_e = host.blas_pseudonormals(pos, idx, sv)
    assert vert.tobytes() == want_v.tobytes() and edge.tobytes() == want_e.tobytes(), name
    assert np.isfinite(vert).all() and np.isfinite(edge).all()
    r.blas_pseudonormals(0, keep[0])                                  # a later call only queues: the same bits
    again_v, again_e = r.read_blas_pseudonormals(0)
    assert again_v.tobytes() == want_v.tobytes() and again_e.tobytes() == want_e.tobytes()
    r.close()


def test_tables_from_hostile_positions_and_an_unaligned_tensor(api):
    import torch
    from pyrtx import host
    from test_gpu_vertex_normals import offset_view
    pos, idx = ns.indexed("icosphere")
    r, sc, meshes = one_mesh_renderer(api, pos, idx)
    keep = make_tables(r, meshes)
    for k, (hostile, _, _) in enumerate(ns.hostile_cases()):
        if k % 2:
            p, whole = offset_view(hostile, f32)                      # starts 4 bytes into its allocation
        else:
            p = dev(hostile)
        torch.cuda.synchronize()
        r.blas_pseudonormals(0, p)
        vert, edge = r.read_blas_pseudonormals(0)
        want_v, want_e = host.blas_pseudonormals(hostile, idx, meshes[0][3])
        assert vert.tobytes() == want_v.tobytes() and edge.tobytes() == want_e.tobytes(), k
        assert np.isfinite(vert).all() and np.isfinite(edge).all()
    r.close()


def test_tables_after_build_and_after_refit(api):
    """alloc_blas + build_blas over the id: the tables follow the slots of that build, pad triangles included; then a refit."""
    import torch
    from pyrtx import host
    from test_blas_refit_cpu import deform
    pos, idx = ns.indexed("Torus")
    idx = np.concatenate([idx[:400], np.full((3, 3), -1, np.int32), idx[400:], [[0, 1, len(pos)]]]).astype(np.int32)
    nrm = host.vertex_normals(pos, idx)
    r, sc, meshes = one_mesh_renderer(api, *ns.indexed("Cube"))
    T, V = len(idx), len(pos)
    r.alloc_blas(0, T, V)
    p, i, n_t = dev(pos), dev(idx, np.int32), dev(nrm)
    torch.cuda.synchronize()
    r.build_blas(0, p, i, n_t)
    r.set_blas_topology(0, i, V)
    r.blas_pseudonormals(0, p)
    blas_t, sv_t, order = host.blas_build_balanced(pos, idx, nrm)
    assert (sv_t < 0).any(), "the build has pad slots"
    vert, edge = r.read_blas_pseudonormals(0)
    want_v, want_e = host.blas_pseudonormals(pos, idx, sv_t)
    assert vert.tobytes() == want_v.tobytes() and edge.tobytes() == want_e.tobytes(), "after build_blas"
    assert (edge[(sv_t < 0).all(1)].view(np.uint32) == 0).all()
    pos2 = deform(pos, "wave", seed=3)
    p2 = dev(pos2)
    torch.cuda.synchronize()
    r.refit_blas(0, p2, r.vertex_normals(0, p2))
    r.blas_pseudonormals(0, p2)
    vert, edge = r.read_blas_pseudonormals(0)
    want_v, want_e = host.blas_pseudonormals(pos2, idx, sv_t)
    assert vert.tobytes() == want_v.tobytes() and edge.tobytes() == want_e.tobytes(), "after refit_blas"
    assert vert.tobytes() != host.blas_pseudonormals(pos, idx, sv_t)[0].tobytes()
    r.close()


# ---- the query ---------------------------------------------------------------------------------------------------------------------------------
_mixed = {}


def mixed(api, monkeypatch=None, grid=None):
    """The mixed frame: icosphere with tables, Diamond without (+ 8), two spheres, a plane.  One shared context, or a fresh one for a knob."""
    if grid is not None:
        monkeypatch.setenv("RTX_QUERY_GRID", str(grid))
    elif "r" in _mixed:
        return _mixed["r"], _mixed["sc"], _mixed["meshes"]
    sc, meshes = ss.rules_scene()
    r = api.Renderer(sc)
    keep = make_tables(r, meshes, ids=(0,))
    if grid is None:
        _mixed.update(r=r, sc=sc, meshes=meshes, keep=keep)
    else:
        r._keep_tables = keep
    return r, sc, meshes


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_query_parity_in_the_mixed_frame(api, n):
    r, sc, meshes = mixed(api)
    rows = mixed_rows(n, seed=n)
    rows_t = dev(rows)
    got = signed_query(api, r, rows_t)
    want = twin(r, sc, meshes, rows, ids=(0,))
    check_channels(got, want, what=f"n = {n}")
    plain = r.query_nearest(rows_t, ALL)
    r.synchronize()
    for name in ALL:
        assert same_bits(plain[name].cpu().numpy(), got[name]).all(), f"{name}: not the channel query_nearest writes"
    if n == 1000:
        ft = got["feature"]
        assert {1, 2, 3, 4, 5, 9, 0} <= set(np.unique(ft).tolist()), np.unique(ft)
        tri = got["triangle_id"] >= 0
        assert ((ft[tri] >= 8) == (got["object_id"][tri] == 1)).all(), "+ 8 for the mesh without tables, and for no other"
        assert same_bits(np.abs(got["signed_distance"]), got["distance"]).all()


def test_one_workgroup_tile_after_tile_sorted_and_masked(api, monkeypatch):
    """RTX_QUERY_GRID=1: one workgroup walks the four tiles of 1000 rows; sorted rounds; the mask as an int and as a tensor."""
    from pyrtx import host
    r, sc, meshes = mixed(api, monkeypatch, grid=1)
    rows = mixed_rows(1000, seed=77)
    rows_t = dev(rows)
    want = twin(r, sc, meshes, rows, ids=(0,))
    for sort in (False, True):
        check_channels(signed_query(api, r, rows_t, sort=sort), want, what=f"grid 1, sort {sort}")
    om = np.array([1, 2, 4, 8, 16], np.uint32)
    r.set_object_masks(om)
    rm = np.where(np.arange(1000) % 5 == 0, 0, np.random.default_rng(2).integers(1, 32, 1000)).astype(np.int32)
    for sort in (False, True):
        got = signed_query(api, r, rows_t, sort=sort, mask=dev(rm, np.int32))
        check_channels(got, twin(r, sc, meshes, rows, ids=(0,), mask=rm.view(np.uint32), object_masks=om), what=f"row masks, sort {sort}")
        assert np.isposinf(got["signed_distance"][rm == 0]).all() and (got["feature"][rm == 0] == 0).all()
        got = signed_query(api, r, rows_t, sort=sort, mask=0b10110)
        check_channels(got, twin(r, sc, meshes, rows, ids=(0,), mask=0b10110, object_masks=om), what=f"int mask, sort {sort}")
        assert not np.isin(got["object_id"], (0, 3)).any()
    r.set_object_masks(None)
    # channel subsets: the two outputs alone, one channel, no feature
    alone = signed_query(api, r, rows_t, channels=())
    assert set(alone) == {"signed_distance", "feature"}
    check_channels(alone, want, what="no channel")
    check_channels(signed_query(api, r, rows_t, channels=("object_id",), feature=False), want, what="one channel, no feature")
    check_channels(signed_query(api, r, rows_t, channels=("uv", "distance"), n=300), want, what="n below the tensor's rows")
    r.close()


def test_chain_scene_reaches_the_spill_region(api):
    """A BVH that is a chain 23 deep: the stack passes RTX_LDS_STACK.  The hand-made mesh has no slot table: every triangle row is + 8."""
    from pyrtx import host
    sc = chain_blas_scene()
    r = api.Renderer(sc)
    rng = np.random.default_rng(12)
    rows = ss.as_rows(np.stack([rng.uniform(-3.5, 3.5, 700), rng.uniform(-1.2, 1.2, 700), rng.uniform(-1.0, 1.0, 700)], 1))
    want = host.query_signed_distance(sc, rows, ALL)
    assert want["stack_max"] > 16, "the spill region is reached"
    for sort in (False, True):
        got = signed_query(api, r, dev(rows), sort=sort)
        check_channels(got, want, what=f"chain, sort {sort}")
    tri = got["triangle_id"] >= 0
    assert tri.sum() > 100 and (got["feature"][tri] >= 9).all() and (got["signed_distance"] < 0).any() and (got["signed_distance"] > 0).any()
    r.close()


@pytest.fixture(scope="module")
def closed(api):
    sc, meshes = ss.closed_scene()
    r = api.Renderer(sc)
    keep = make_tables(r, meshes)
    yield r, sc, meshes
    r.close()


def test_closed_scene_and_update_instances(api, closed):
    """The six posed instances (one mirrored) with tables for every mesh; then new random poses through update_instances."""
    import torch
    r, sc, meshes = closed
    rng = np.random.default_rng(21)
    rows = ss.as_rows(ss.uniform_rows(sc, meshes, 600, rng))
    got = signed_query(api, r, dev(rows))
    check_channels(got, twin(r, sc, meshes, rows, ids=range(len(meshes))), what="as set")
    assert (got["feature"] < 8).all() and set(np.unique(got["object_id"])) == set(range(6))
    rot = dev(ss.random_quaternions(6, rng))
    pos = dev(np.stack([np.arange(6) * 3.5, rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 6)], 1))      # 3.5 apart: no two solids overlap
    torch.cuda.synchronize()
    r.update_instances(pos, rot)
    rows = ss.as_rows(np.stack([rng.uniform(-2, 19.5, 600), rng.uniform(-1.5, 1.5, 600), rng.uniform(-1.5, 1.5, 600)], 1))      # the solids fill about a tenth of this box
    got = signed_query(api, r, dev(rows), sort=True)
    check_channels(got, twin(r, sc, meshes, rows, ids=range(len(meshes))), what="after update_instances")
    assert (got["signed_distance"] < 0).sum() > 10


def test_sign_oracle_on_the_device(api, closed):
    """300 rows around the posed Rock and Torus (wherever the previous poses left them) against the float64 winding number of the posed
    triangles read back from the context, under the leave-out rule and the 2 % cap of the CPU test."""
    r, sc, meshes = closed
    inst, nodes, idx = r.read_frame_state()

    class Frame:
        instances = inst
    rng = np.random.default_rng(33)
    tris, owner = ss.posed_triangles(Frame, meshes)
    pts = []
    for i in (2, 3):
        q = tris[owner == i].reshape(-1, 3)
        c, h = (q.min(0) + q.max(0)) / 2, (q.max(0) - q.min(0)) / 2 * 1.25
        pts.append(rng.uniform(c - h, c + h, (150, 3)))
    rows = ss.as_rows(np.concatenate(pts))
    got = signed_query(api, r, dev(rows), channels=("object_id",))
    inside = np.abs(ss.winding_number(rows[:, :3], tris)) > 0.5                   # the solids do not overlap: the union's number is the owner's
    left_out, _ = ss.undetermined(Frame, meshes, rows)
    print(f"{len(rows)} rows, {int(left_out.sum())} left out, {int(inside.sum())} inside")
    assert left_out.mean() <= 0.02 and inside.sum() > 20
    wrong = ~left_out & ((got["signed_distance"] < 0) != inside)
    assert not wrong.any(), (np.nonzero(wrong)[0], got["feature"][wrong], got["object_id"][wrong])


# ---- state -------------------------------------------------------------------------------------------------------------------------------------
def test_alloc_blas_over_the_id_drops_the_tables(api):
    import torch
    from pyrtx import host
    sc, meshes = ss.rules_scene()
    r = api.Renderer(sc)
    keep = make_tables(r, meshes)
    rows = mixed_rows(500, seed=5)
    rows_t = dev(rows)
    before = signed_query(api, r, rows_t)
    assert (before["feature"] < 8).all()
    pos, idx = meshes[0][0], meshes[0][1]
    nrm = host.vertex_normals(pos, idx)
    r.query_signed_distance(rows_t, ALL)                               # queued: the swap below waits for it
    r.alloc_blas(0, len(idx), len(pos))
    assert r.lib.rtx_read_blas_pseudonormals(r.ctx, 0, before["distance"].ctypes.data, None) == STATE
    p, i, n_t = dev(pos), dev(idx, np.int32), dev(nrm)
    torch.cuda.synchronize()
    r.build_blas(0, p, i, n_t)
    got = signed_query(api, r, rows_t)
    tri = got["triangle_id"] >= 0
    assert ((got["feature"][tri] >= 8) == (got["object_id"][tri] == 0)).all() and (got["object_id"][tri] == 0).sum() > 20
    arrays, blas = read_back(r, sc)
    want = host.query_signed_distance(arrays, rows, ALL, blas=blas, pseudonormals={1: r.read_blas_pseudonormals(1) + (meshes[1][3],)})
    check_channels(got, want, what="after alloc_blas + build_blas over id 0")
    # tables again, over the slots of the build
    r.set_blas_topology(0, i, len(pos))
    r.blas_pseudonormals(0, p)
    got = signed_query(api, r, rows_t)
    assert (got["feature"] < 8).all()
    sv_t = host.blas_build_balanced(pos, idx, nrm)[1]
    want = host.query_signed_distance(arrays, rows, ALL, blas=blas, pseudonormals={0: r.read_blas_pseudonormals(0) + (sv_t,), 1: r.read_blas_pseudonormals(1) + (meshes[1][3],)})
    check_channels(got, want, what="tables over the new slots")
    r.close()


def test_error_codes_in_order_and_a_valid_query_after_them(api):
    import torch
    r, sc, meshes = one_mesh_renderer(api, *ns.indexed("Diamond"))
    pos, idx, _, sv = meshes[0]
    V = len(pos)
    lib, ctx = r.lib, r.ctx
    p, i = dev(pos), dev(idx, np.int32)
    rows = mixed_rows(100, seed=1)
    rows_t = dev(rows)
    sd, ft = guarded(100, 1, np.float32)[0], guarded(100, 1, np.int32)[0]
    dist = guarded(100, 1, np.float32)[0]
    torch.cuda.synchronize()
    pn = lambda b, ptr: lib.rtx_blas_pseudonormals(ctx, b, ptr)
    assert lib.rtx_blas_pseudonormals(None, 0, p.data_ptr()) == INVALID
    assert pn(0, None) == INVALID and pn(0, p.data_ptr() + 2) == INVALID
    assert pn(0, p.data_ptr()) == STATE and pn(-1, p.data_ptr()) == STATE and pn(99, p.data_ptr()) == STATE, "no topology allocated"
    assert lib.rtx_alloc_blas_topology(ctx, 0, len(idx), V) == 0
    assert pn(0, p.data_ptr()) == STATE, "no topology set"
    r.set_blas_topology(0, i, V)                                      # through the Renderer, which then knows the shape it reads back
    assert pn(0, p.data_ptr()) == STATE, "no vertices bound"
    r.bind_blas_vertices(0, sv, V + 1)
    assert pn(0, p.data_ptr()) == INVALID, "the topology's vertex_count is not the bound one"
    r.bind_blas_vertices(0, sv, V)
    assert lib.rtx_read_blas_pseudonormals(ctx, 0, None, None) == INVALID
    assert lib.rtx_read_blas_pseudonormals(ctx, 0, sd.data_ptr(), None) == STATE, "no tables yet"
    buf = api.RtxQueryBuffers(); buf.distance = dist.data_ptr()
    q = lambda pts, n, ch, out, s, f, fl, flt=None: lib.rtx_query_signed_distance(ctx, pts, n, ch, out, s, f, fl, flt)
    P, S_, F = rows_t.data_ptr(), sd.data_ptr(), ft.data_ptr()
    assert lib.rtx_query_signed_distance(None, P, 100, 1, C.byref(buf), S_, F, 0, None) == INVALID
    assert q(P, 100, 8, C.byref(buf), S_, F, 0) == INVALID, "a bit outside RTX_QUERY_ALL"
    assert q(P, 100, 1, C.byref(buf), None, F, 0) == INVALID, "signed_dev is required"
    assert q(P, 100, 1, C.byref(buf), S_ + 2, F, 0) == INVALID and q(P, 100, 1, C.byref(buf), S_, F + 1, 0) == INVALID
    assert q(None, 100, 1, C.byref(buf), S_, F, 0) == INVALID and q(P, 100, 1, None, S_, F, 0) == INVALID and q(P, 0, 1, C.byref(buf), S_, F, 0) == INVALID
    assert q(P, 100, 1, C.byref(buf), S_, F, 1) == INVALID, "a flag other than RTX_QUERY_SORT"
    assert b"RTX_QUERY_SORT" in lib.rtx_last_error(ctx)
    r.synchronize()
    assert bool((sd.view(torch.int32) == PATTERN).all()) and bool((ft == PATTERN).all()) and bool((dist.view(torch.int32) == PATTERN).all()), "an error queues nothing"
    # and now the valid calls
    assert q(P, 100, 0, None, S_, None, 0) == 0, "no channel, no buffers, no feature"
    assert pn(0, p.data_ptr()) == 0
    got = signed_query(api, r, rows_t)
    check_channels(got, twin(r, sc, meshes, rows, ids=(0,)), what="after the errors")
    r.synchronize()
    assert same_bits(np.abs(got["signed_distance"]), np.abs(sd.cpu().numpy())).all(), "the tables change signs only"
    r.close()


def test_state_and_limit_errors_in_the_documented_order(api):
    """After the argument errors of rtx_query_signed_distance: RTX_ERR_STATE before rtx_set_frame and in heat-map mode, RTX_ERR_LIMIT for the
    stack rule of a render call and for the walk's own rule (the recipe of tests/test_gpu_query_nearest.py for the unsigned call), then the
    state rule of the filtered queries: a table set for other counts than the frame's.  A filter WITHOUT a table is no error (include/rtx.h,
    filtered queries: every object's mask is then all ones).  On each such context the argument errors still come first; nothing is queued."""
    import copy
    import torch
    from pyrtx import host
    sc, meshes = ss.rules_scene()
    r = api.Renderer(sc)
    lib, n = r.lib, 100
    rows = mixed_rows(n, seed=3)
    rows_t = dev(rows)
    sd, ft, dist = guarded(n, 1, np.float32)[0], guarded(n, 1, np.int32)[0], guarded(n, 1, np.float32)[0]
    buf = api.RtxQueryBuffers(); buf.distance = dist.data_ptr()
    filt = api.RtxQueryFilter(None, 0b11)
    torch.cuda.synchronize()
    P, S_, F, B, FL, D = rows_t.data_ptr(), sd.data_ptr(), ft.data_ptr(), C.byref(buf), C.byref(filt), api.RTX_QUERY_DISTANCE
    q = lambda ctx, ch=D, out=B, s=S_, flags=0, flt=None, pts=P, m=n: lib.rtx_query_signed_distance(ctx, pts, m, ch, out, s, F, flags, flt)

    def arguments_first(ctx, what):
        assert q(ctx, ch=D | 8) == INVALID and q(ctx, s=None) == INVALID and q(ctx, out=None) == INVALID and q(ctx, m=0) == INVALID, what
        assert q(ctx, pts=None) == INVALID and q(ctx, flags=1) == INVALID and q(ctx, flags=64 | 256) == INVALID, what
        assert q(ctx, ch=D | 8, flt=FL) == INVALID and q(ctx, flags=1, flt=FL) == INVALID, what
    empty = api.Renderer(sc, upload=False)
    assert q(empty.ctx) == STATE and q(empty.ctx, ch=0, out=None) == STATE and q(empty.ctx, flt=FL) == STATE, "before rtx_set_frame"
    assert b"rtx_query_signed_distance" in lib.rtx_last_error(empty.ctx)
    arguments_first(empty.ctx, "before rtx_set_frame")
    heat = copy.deepcopy(sc); heat.config["heatmap"] = 1
    rh = api.Renderer(heat)
    assert q(rh.ctx) == STATE and q(rh.ctx, ch=0, out=None) == STATE, "heat-map mode"
    arguments_first(rh.ctx, "heat-map mode")
    shallow, _ = util.load_golden("monkey_small"); shallow = copy.deepcopy(shallow); shallow.config["stack_size"] = 3
    rs = api.Renderer(shallow)
    assert q(rs.ctx) == LIMIT and q(rs.ctx, ch=0, out=None) == LIMIT and q(rs.ctx, flt=FL) == LIMIT, "the stack rule of a render call"
    arguments_first(rs.ctx, "a shallow stack")
    # the walk's own rule: the chain's deepest inner node is at depth 22; under a TLAS of one leaf the descent needs 23 entries, under a TLAS
    # of three instances (inner depth 1) 25, against a stack_size of 24
    chain = chain_blas_scene(); chain.config["stack_size"] = 24
    rc = api.Renderer(chain)
    assert q(rc.ctx) == 0
    three = copy.deepcopy(chain)
    three.instances = np.concatenate([chain.instances] * 3)
    root = chain.blas[0].nodes[0]
    boxes, centres = [], []
    for k in range(3):
        three.instances["world"][k][3] += 9.0 * k; three.instances["world_inv"][k][3] -= 9.0 * k
        boxes.append(np.concatenate([root["aabb_min"] + (9 * k, 0, 0), root["aabb_max"] + (9 * k, 0, 0)])); centres.append((9.0 * k, 0, 0))
    three.tlas_nodes, three.tlas_indices = host.tlas_build_balanced(np.array(centres, f32), np.array(boxes, f32))
    rt = api.Renderer(three)
    rt.render()                                                        # rays are served
    assert q(rt.ctx) == LIMIT and q(rt.ctx, ch=0, out=None) == LIMIT, "(1 + 1) + (22 + 1) = 25 entries against a stack_size of 24"
    assert b"stack" in lib.rtx_last_error(rt.ctx)
    arguments_first(rt.ctx, "the walk's stack rule")
    # a frame with a scaled instance: RTX_ERR_STATE after the checks of a render call (a shallow stack stays RTX_ERR_LIMIT) and before the walk's
    # own stack rule (the three chains, enlarged by 2, are no longer RTX_ERR_LIMIT); the argument checks still come first; nothing is queued
    import affineset
    rn = api.Renderer(affineset.with_linear(three, [affineset.LINEAR["uniform2"]]))
    rsn = api.Renderer(affineset.with_linear(shallow, [affineset.LINEAR["uniform2"]]))
    assert q(rn.ctx) == STATE and q(rn.ctx, ch=0, out=None) == STATE and q(rn.ctx, flt=FL) == STATE, "a scaled instance, before the walk's stack rule"
    assert b"rigid" in lib.rtx_last_error(rn.ctx) and q(rsn.ctx) == LIMIT
    arguments_first(rn.ctx, "a scaled instance")
    rn.synchronize(); rsn.synchronize()
    rc.synchronize()
    sd.view(torch.int32).fill_(PATTERN)                                # the valid call on the chain wrote it
    torch.cuda.synchronize()
    # the filtered form on the good context: no table is no error; a table for other counts is, after the argument errors
    assert q(r.ctx, flt=FL) == 0, "a filter without a table: every object's mask is all ones"
    r.synchronize()
    no_table = sd.cpu().numpy().copy()
    sd.view(torch.int32).fill_(PATTERN); ft.fill_(PATTERN); dist.view(torch.int32).fill_(PATTERN)
    torch.cuda.synchronize()
    r.set_object_masks(np.array([1, 2, 4, 8, 16], np.uint32))
    fewer = copy.copy(sc); fewer.planes = sc.planes[:0].copy()
    r.set_frame(fewer)
    assert q(r.ctx, flt=FL) == STATE and q(r.ctx, ch=0, out=None, flt=FL) == STATE, "the object masks were set for other counts"
    assert b"object masks" in lib.rtx_last_error(r.ctx)
    arguments_first(r.ctx, "stale object masks")
    assert q(r.ctx) == 0, "a NULL filter is the unfiltered call: it goes on"
    for other in (empty, rh, rs, rc, rt, r):
        other.synchronize()
    assert not bool((ft == PATTERN).any()) and not bool((dist.view(torch.int32) == PATTERN).any()), "that last call ran"
    r.set_frame(sc)
    r.set_object_masks(None)
    sd.view(torch.int32).fill_(PATTERN); ft.fill_(PATTERN); dist.view(torch.int32).fill_(PATTERN)
    torch.cuda.synchronize()
    for ctx in (empty.ctx, rh.ctx, rs.ctx, rt.ctx):
        assert q(ctx) != 0
    for other in (empty, rh, rs, rt):
        other.synchronize()
    assert bool((sd.view(torch.int32) == PATTERN).all()) and bool((ft == PATTERN).all()) and bool((dist.view(torch.int32) == PATTERN).all()), "an error queues nothing"
    # and a valid query after them, equal to the filtered call without a table where the row masks hide nothing
    got = signed_query(api, r, rows_t)
    want = host.query_signed_distance(sc, rows, ALL)
    check_channels(got, want, what="after the errors")
    assert same_bits(got["signed_distance"], no_table).all(), "row mask 0b11 without a table hides nothing"
    for other in (empty, rh, rs, rc, rt, r):
        other.close()


def test_upload_over_the_id_and_a_new_topology_drop_the_tables(api):
    """The other two routes that drop the tables: rtx_upload_blas over the id (commit_blas), and rtx_alloc_blas_topology over it (the tables
    were made from the replaced topology's lists).  The next query reports + 8 for that mesh and for no other."""
    import torch
    from pyrtx import host
    sc, meshes = ss.rules_scene()
    r = api.Renderer(sc)
    keep = make_tables(r, meshes)
    rows = mixed_rows(500, seed=6)
    rows_t = dev(rows)
    assert (signed_query(api, r, rows_t)["feature"] < 8).all()
    scratch = np.zeros(4 * len(meshes[0][0]), f32)

    def only(with_tables, what):
        got = signed_query(api, r, rows_t)
        tri = got["triangle_id"] >= 0
        for b in (0, 1):
            owned = tri & (got["object_id"] == b)
            assert owned.sum() > 20 and ((got["feature"][owned] < 8) == (b in with_tables)).all(), (what, b)
        check_channels(got, twin(r, sc, meshes, rows, ids=with_tables), what=what)
    r.query_signed_distance(rows_t, ALL)                               # queued: the swap below waits for it
    b = sc.blas[0]
    nodes, hot, cold = np.ascontiguousarray(b.nodes), np.ascontiguousarray(b.tri_hot), np.ascontiguousarray(b.tri_cold)
    assert r.lib.rtx_upload_blas(r.ctx, 0, nodes.ctypes.data, len(nodes), hot.ctypes.data, cold.ctypes.data, len(hot), b.material_offset) == 0
    assert r.lib.rtx_read_blas_pseudonormals(r.ctx, 0, scratch.ctypes.data, None) == STATE
    only((1,), "after rtx_upload_blas over id 0")
    r.query_signed_distance(rows_t, ALL)
    assert r.lib.rtx_alloc_blas_topology(r.ctx, 1, len(meshes[1][1]), len(meshes[1][0])) == 0
    assert r.lib.rtx_read_blas_pseudonormals(r.ctx, 1, scratch.ctypes.data, None) == STATE
    only((), "after rtx_alloc_blas_topology over id 1")
    keep += make_tables(r, meshes)                                     # and back: bind, topology, tables for both
    only((0, 1), "tables made again")
    r.close()


def test_queued_between_frames_without_a_wait(api):
    """frame, tables, signed query, nearest query, frame — nothing synchronised in between: the frames are those of a context that renders
    only, the answers those of the twin, and rtx_get_stats reports the frame's numbers."""
    import torch
    sc, meshes = ss.rules_scene()
    ref = api.Renderer(sc)
    ref.render_async()
    want_frame = ref.render()
    ref.close()
    r = api.Renderer(sc)
    rows = mixed_rows(700, seed=9)
    rows_t = dev(rows)
    keep = [dev(meshes[0][0]), dev(meshes[0][1], np.int32)]
    torch.cuda.synchronize()
    r.bind_blas_vertices(0, meshes[0][3], len(meshes[0][0]))
    r.render_async()
    r.set_blas_topology(0, keep[1], len(meshes[0][0]))
    r.blas_pseudonormals(0, keep[0])
    a = r.query_signed_distance(rows_t, ALL, feature=True, sort=True)
    b = r.query_nearest(rows_t, ALL)
    r.blas_pseudonormals(0, keep[0])
    c = r.query_signed_distance(rows_t, ("distance",), feature=True)
    got_frame = r.render()
    assert got_frame["packed"].tobytes() == want_frame["packed"].tobytes() and got_frame["rgb"].tobytes() == want_frame["rgb"].tobytes()
    assert got_frame["stats"] == want_frame["stats"]
    want = twin(r, sc, meshes, rows, ids=(0,))
    check_channels({k: v.cpu().numpy() for k, v in a.items()}, want, what="first query")
    check_channels({k: v.cpu().numpy() for k, v in b.items()}, want, what="query_nearest in between")
    check_channels({k: v.cpu().numpy() for k, v in c.items()}, want, what="second query")
    r.close()
