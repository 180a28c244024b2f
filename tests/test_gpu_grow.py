"""A context that grows after its first frame: new BLAS, texture ids, a larger material table, a sky of another size — and no rtx_set_frame
that the contract does not ask for (include/rtx.h, "scene data that lives across frames": an upload or alloc takes effect at the next render
or query call).  Every one of these makes a device table of the context larger, so the table moves; the scene the kernels receive by value
must name the table the context holds when the call is made (csrc/rtx_hostmem.h, bind_tables / replace_table; the rule itself is pinned on
the CPU by csrc/hostmem_check.cpp, tests/test_hostmem_cpu.py).

Everything is bit for bit (float arrays as uint32, stats equal); there is no tolerance in this file.  Every frame is compared with a FRESH
context that received the final state through plain uploads plus set_frame, and the tiles entry point with the oracle as well; every query
with its host twin (nearest, hits, sweep, signed distance) or the oracle (closest, occluded), on the arrays the test itself holds.  Scenes:
the `cube` golden at 64 x 64 for the mesh cases, a 64 x 48 cut of `materials_aniso` (textures, dielectrics, rays that reach the sky) for
materials, textures and sky; queries of at most 256 rows.  All calls are legal calls with finite data; the one refusal (a material table
that no longer covers a triangle's id) is the host's validation.

  1  a BLAS id nobody refers to, uploaded under ids 1, 2 and 7: all four render entry points and all six queries answer as before
  2  the same through alloc_blas: unbuilt, built, then update_instances (it reads the BLAS table) and a set_frame that uses the new id
  3  a new texture id (dense, then sparse), used through a material re-upload of the same count, and back
  4  a larger material table, unchanged in front, then changed; a table that is too short is refused by render and query alike
  5  a sky of 32, 128 and 64 texels a side; rtx_update_sky follows the size
  6  1, 3 and 5 with RTX_GRAPH=1: three identical calls before the growth and three after
  7  a frame queued before the growth keeps the state it was queued with
  8  three contexts growing different tables in turn
  9  test_sequences_*: the seeded edit sequences of tests/growset.py on one long-lived context, every observation against a fresh context,
     the twins or the oracle; once more with RTX_GRAPH=1, every observation three times
"""
import copy

import numpy as np
import pytest

import growset
import hitset
import pointset
import sweepset
import util
from test_blas_build_cpu import soup, twin as balanced_twin
from test_gpu_query import check_channels, expected as oracle_closest, zero_diff
from test_gpu_query_hits import check as check_hits
from test_gpu_ray_views import assert_same, camera_rays
from test_gpu_replace import assert_blas, cube_scene, monkey_blas
from test_gpu_views import camera_set

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL = hitset.ALL
STATE = 5
SEEDS = growset.default_seeds()


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def dev(a, dtype=f32):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()
    torch.cuda.synchronize()                                 # torch copies on its own stream: done before a library call reads the tensor
    return t


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
def same_out(got, want, what):
    """every array of `want` bit for bit, the ray counts equal"""
    for name, w in want.items():
        if name == "stats":
            assert got["stats"] == w, (what, got["stats"], w)
        elif name != "work":
            assert_same(np.asarray(got[name]), np.asarray(w), f"{what}: {name}")


def differs(a, b):
    return not np.array_equal(a["packed"], b["packed"])


def frame(r, api, kind, sc, **flags):
    """one render observation through the entry point `kind`"""
    if kind == "render":
        return r.render(**flags)
    if kind == "render_views":
        r.set_views(camera_set(sc)[:2])
        return r.render_views(**flags)
    if kind == "render_rays":
        r.set_rays(camera_rays(api, sc, sc.camera))
        return r.render_rays(**flags)
    return r.render_aovs(tuple(api.AOV_CHANNELS), **flags)


def all_frames(r, api, sc):
    return {kind: frame(r, api, kind, sc) for kind in growset.RENDERS}


_refs = {}


def reference(api, key, sc):
    """The frame of the state `sc` through every entry point, from a fresh context that got it by plain uploads and one set_frame; the tiles
    frame is the oracle's too.  Once per key and run."""
    if key not in _refs:
        import orc
        fresh = api.Renderer(sc)
        out = all_frames(fresh, api, sc)
        fresh.close()
        same_out(out["render"], orc.OracleScene(sc).render(threads=8), f"{key}: fresh context vs oracle")
        _refs[key] = out
    return _refs[key]


# ---- queries ---------------------------------------------------------------------------------------------------------------------------
def ask(r, kind, rows_t, sort=False, mask=None):
    """one query observation -> {name: tensor}"""
    if hasattr(mask, "dtype"):
        mask = dev(mask, np.int32)
    if kind == "closest":
        return r.query_closest(rows_t, ALL, sort=sort)
    if kind == "occluded":
        return {"occluded": r.query_occluded(rows_t, sort=sort)}
    if kind == "nearest":
        return r.query_nearest(rows_t, ALL, sort=sort, mask=mask)
    if kind == "hits":
        return r.query_hits(rows_t, 4, ALL, sort=sort, mask=mask)
    if kind == "sweep":
        return r.query_sweep(rows_t, ALL, sort=sort, mask=mask)
    return r.query_signed_distance(rows_t, ALL, sort=sort, mask=mask, feature=True)


def answers(kind, sc, rows, mask=None, object_masks=None):
    """the same from the host: the oracle for the ray queries, the twins for the walk queries (no mesh has pseudonormal tables)"""
    from pyrtx import host
    if kind in ("closest", "occluded"):
        import orc
        o = orc.OracleScene(sc)
        if kind == "closest":
            return oracle_closest(o, rows)
        return {"occluded": o.trace_any(zero_diff(rows[:, :6]), rows[:, 6]).astype(np.int32)}
    if mask is None:
        object_masks = None                                  # the unfiltered call, whatever table the context holds
    kw = {"mask": mask, "object_masks": object_masks}
    if kind == "nearest":
        return host.query_nearest(sc, rows, ALL, **kw)
    if kind == "hits":
        return host.query_hits(sc, rows, 4, ALL, **kw)
    if kind == "sweep":
        return host.query_sweep(sc, rows, ALL, **kw)
    return host.query_signed_distance(sc, rows, ALL, **kw)


def check_answers(kind, got, want, what):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    if kind == "occluded":
        assert np.array_equal(got["occluded"] != 0, want["occluded"] != 0), (what, int(((got["occluded"] != 0) != (want["occluded"] != 0)).sum()))
    elif kind == "hits":
        check_hits(got, want, None, what)
    else:
        check_channels(got, want, None, what)
    return got


def finite_rows(rows, n=256):
    return np.ascontiguousarray(rows[~np.isnan(rows).any(axis=1)][:n], f32)


class QuerySet:
    """At most 256 rows for each of the six queries on `sc` and what the host answers: pinhole rays of the camera and the segment generator's
    rays (edges, surface points, box planes); the point, segment and sweep generators of the kernels' own test files."""

    def __init__(self, api, sc, seed):
        rng = np.random.default_rng([seed, 77])
        px = rng.choice(sc.width * sc.height, 160, replace=False)
        segs = finite_rows(hitset.generate(sc, 10, seed)[0])
        rays = np.concatenate([api.pinhole_rays(sc.camera[0], sc.width, sc.height).reshape(-1, 18)[px, :6], segs[:, :6]])
        far = rng.choice(f32([0.5, 2.0, 6.0, 30.0, np.inf]), (len(rays), 1))
        pts = finite_rows(pointset.generate(sc, 200, seed)[0])
        self.rows = {"closest": finite_rows(rays), "occluded": finite_rows(np.concatenate([rays, far], axis=1)), "nearest": pts, "signed": pts,
                     "hits": segs, "sweep": finite_rows(sweepset.generate(sc, 200, seed)[0])}
        assert all(64 < len(v) <= 256 for v in self.rows.values()), {k: len(v) for k, v in self.rows.items()}
        self.want = {kind: answers(kind, sc, rows) for kind, rows in self.rows.items()}
        assert np.isfinite(self.want["closest"]["distance"]).sum() > 16 and np.isfinite(self.want["nearest"]["distance"]).sum() > 16
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = {kind: dev(rows) for kind, rows in self.rows.items()}
        return self._dev

    def check(self, r, what, sort=False):
        return {kind: check_answers(kind, ask(r, kind, self.dev[kind], sort), self.want[kind], f"{what}: {kind}") for kind in growset.QUERIES}


def same_answers(a, b, what):
    for kind in a:
        for name in a[kind]:
            assert_same(a[kind][name], b[kind][name], f"{what}: {kind} {name}")


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_blas_id_nobody_refers_to(api):
    sc = cube_scene()
    mk = monkey_blas(sc)
    r = api.Renderer(sc)
    A = all_frames(r, api, sc)
    assert len(np.unique(A["render"]["packed"])) > 1                              # the cube is in view
    for kind, ref in reference(api, "cube", sc).items():
        same_out(A[kind], ref, f"frame A, {kind}")
    qs = QuerySet(api, sc, 3)
    before = qs.check(r, "before any growth")
    for k, bid in enumerate((1, 2, 7)):                                          # 7: a sparse id; the table grows every time
        r.upload_blas(bid, mk)
        what = f"after rtx_upload_blas under id {bid}"
        out = all_frames(r, api, sc)
        for kind in growset.RENDERS:
            same_out(out[kind], A[kind], f"{what}, {kind}")
        same_answers(qs.check(r, what, sort=bool(k & 1)), before, what)
        assert_blas(r.read_blas(0), sc.blas[0], what)
        assert_blas(r.read_blas(bid), mk, what)
    r.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def ahead_of(sc, distance, aside=0.0):
    cam = sc.camera[0]
    d = (cam["rotated_top_left_corner"] + f32(sc.width / 2) * cam["rotated_x_axis"] + f32(sc.height / 2) * cam["rotated_y_axis"]).astype(np.float64)
    x = cam["rotated_x_axis"].astype(np.float64)
    return (cam["position"] + distance * d / np.linalg.norm(d) + aside * x / np.linalg.norm(x)).astype(f32)


def test_a_new_id_through_alloc_blas(api):
    import torch
    from pyrtx import host
    from pyrtx import scene_io as sio
    sc = cube_scene()
    pos, idx, nrm, uv, mid = soup(257, 7)
    pos = (pos * f32(0.25)).astype(f32)
    tw, sv, order = balanced_twin(pos, idx, nrm, uv, mid)
    r = api.Renderer(sc)
    A = r.render()
    same_out(A, reference(api, "cube", sc)["render"], "frame A")
    r.alloc_blas(1, len(idx), len(pos), mid)
    same_out(r.render(), A, "after rtx_alloc_blas of a new id (empty, legal to render)")
    keep = (dev(pos), dev(idx, np.int32), dev(nrm), dev(uv))
    r.build_blas(1, *keep)
    same_out(r.render(), A, "after rtx_build_blas of the new id")
    assert_blas(r.read_blas(1), tw, "the built mesh")
    assert_blas(r.read_blas(0), sc.blas[0], "its neighbour")

    # rtx_update_instances reads the BLAS table (the root boxes) without a set_frame since the table moved
    p1 = ahead_of(sc, 6.0, 0.5)[None]; q1 = f32([[0.18257419, 0.36514837, 0.54772256, 0.73029674]])
    moved = copy.copy(sc)
    moved.instances, moved.tlas_nodes, moved.tlas_indices = host.scene_update_balanced(sc, p1, q1)
    keep += (dev(p1), dev(q1))
    r.update_instances(keep[-2], keep[-1])
    for g, w, name in zip(r.read_frame_state(), (moved.instances, moved.tlas_nodes, moved.tlas_indices), ("instances", "tlas nodes", "tlas indices")):
        assert g.tobytes() == w.tobytes(), f"after rtx_update_instances: {name}"
    B = r.render()
    same_out(B, reference(api, "cube moved", moved)["render"], "after rtx_update_instances")
    assert differs(B, A) and len(np.unique(B["packed"])) > 1

    # a frame that uses the new id: the fresh context got the twin's BLAS through rtx_upload_blas
    both = copy.copy(sc)
    both.blas = [sc.blas[0], tw]
    both.instances = np.zeros(2, sio.INSTANCE); both.instances["blas_id"] = (0, 1)
    p2 = np.stack([p1[0], ahead_of(sc, 3.5, -0.4)]); q2 = np.concatenate([q1, f32([[0, 0, 0, 1]])])
    both.instances, both.tlas_nodes, both.tlas_indices = host.scene_update_balanced(both, p2, q2)
    r.set_frame(both)
    D = r.render()
    same_out(D, reference(api, "cube and soup", both)["render"], "after set_frame with an instance of the new id")
    assert differs(D, B)
    torch.cuda.synchronize()
    r.close()


# ---- the growth of each table on the materials scene: stages of (calls, the state after them) ---------------------------------------------
def textured(sc):
    """the first material with a texture (the plane's)"""
    return int(np.flatnonzero(sc.materials["texture_id"] >= 0)[0])


def with_texture(sc, tid, tex, material):
    """sc with `tex` under id tid (ids between: one black texel each, referred to by nobody) and `material` switched to it"""
    from pyrtx import host
    out = copy.copy(sc)
    out.textures = list(sc.textures) + [host.texture_with_mips(np.zeros((1, 1, 3), f32)) for _ in range(len(sc.textures), tid)] + [tex]
    out.materials = sc.materials.copy()
    out.materials["texture_id"][material] = tid
    return out


def new_level0(seed=5):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (16, 64, 3)).astype(f32)


def padded_materials(sc, extra, seed=9):
    rng = np.random.default_rng(seed)
    more = np.zeros(extra, sc.materials.dtype)
    more["diffuse"] = rng.uniform(0, 1, (extra, 3)).astype(f32); more["texture_id"] = -1; more["index_of_refraction"] = 1.0
    return np.concatenate([sc.materials, more])


def recipe(table, sc, keep):
    """-> [(key, [call(r), ...], the scene after the calls), ...]"""
    from pyrtx import host
    if table == "blas":                                       # two ids nobody refers to; then the mesh of id 3 replaced and one more new id
        mk = copy.copy(util.load_golden("monkey_small")[0].blas[0])
        mk.material_offset = sc.blas[3].material_offset
        n = len(sc.blas)
        grown = copy.copy(sc); grown.blas = list(sc.blas); grown.blas[3] = mk
        return [("materials", [lambda r: r.upload_blas(n, mk), lambda r: r.upload_blas(n + 6, mk)], sc),
                ("materials blas 3", [lambda r: r.upload_blas(3, mk), lambda r: r.upload_blas(n + 1, mk)], grown)]
    if table == "textures":                                   # a sparse new id, updated from a tensor, used through a material re-upload
        tid, level0 = len(sc.textures) + 5, new_level0()
        grown = with_texture(sc, tid, host.texture_with_mips(level0), textured(sc))
        t = dev(level0); keep.append(t)
        return [("materials texture", [lambda r: r.alloc_texture(tid, 64, 16), lambda r: r.update_texture(tid, t),
                                       lambda r: r.upload_materials(grown.materials)], grown)]
    if table == "materials":                                  # a larger table, one of the old entries changed
        grown = copy.copy(sc)
        grown.materials = padded_materials(sc, 40); grown.materials["reflection"][textured(sc)] = (0.6, 0.1, 0.4)
        return [("materials", [lambda r: r.upload_materials(padded_materials(sc, 3))], sc),
                ("materials 40 more", [lambda r: r.upload_materials(grown.materials)], grown)]
    grown = copy.copy(sc); grown.sky = np.ascontiguousarray(host.synthetic_sky(128) * f32(0.5))
    return [("materials sky 128 at half the light", [lambda r: r.upload_sky(host.synthetic_sky(32)), lambda r: r.upload_sky(grown.sky)], grown)]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_new_texture_id_used_without_set_frame(api):
    from pyrtx import host
    sc = growset.materials_scene()
    level0 = new_level0()
    tex, m = host.texture_with_mips(level0), textured(sc)
    r = api.Renderer(sc)
    A = r.render()
    same_out(A, reference(api, "materials", sc)["render"], "frame A")
    t = dev(level0)
    for tid in (len(sc.textures), len(sc.textures) + 5):
        r.alloc_texture(tid, 64, 16)
        same_out(r.render(), A, f"after rtx_alloc_texture of id {tid} (black, legal to render)")
        r.update_texture(tid, t)
        grown = with_texture(sc, tid, tex, m)
        r.upload_materials(grown.materials)
        B = r.render()
        same_out(B, reference(api, f"materials texture {tid}", grown)["render"], f"texture id {tid} through material {m}")
        assert differs(B, A), "the new texture is meant to show"
        got = r.read_texture(tid)
        assert got.desc.tobytes() == tex.desc.tobytes() and got.texels.tobytes() == tex.texels.tobytes()
        r.upload_materials(sc.materials)
        same_out(r.render(), A, f"switched back from texture id {tid}")
    r.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_larger_material_table(api):
    sc = growset.materials_scene()
    count = len(sc.materials)
    r = api.Renderer(sc)
    A = r.render()
    same_out(A, reference(api, "materials", sc)["render"], "frame A")
    qs = QuerySet(api, sc, 4)
    qs.check(r, "before any growth")
    for extra in (3, 40):
        r.upload_materials(padded_materials(sc, extra))
        same_out(r.render(), A, f"{count} + {extra} materials, the first {count} unchanged")
        qs.check(r, f"{count} + {extra} materials", sort=extra == 40)
    (_, calls, grown), = recipe("materials", sc, [])[1:]
    calls[0](r)
    B = r.render()
    same_out(B, reference(api, "materials 40 more", grown)["render"], "one of the old entries changed")
    assert differs(B, A)
    # a table that no longer covers the plane's material: refused by the next render and the next query, nothing is launched
    assert int(sc.planes["material_id"].max()) >= 7
    r.upload_materials(sc.materials[:7])
    with pytest.raises(api.RtxError) as e:
        r.render()
    assert e.value.code == STATE
    with pytest.raises(api.RtxError) as e:
        r.query_closest(qs.dev["closest"], ALL)
    assert e.value.code == STATE
    with pytest.raises(api.RtxError) as e:
        r.query_nearest(qs.dev["nearest"], ALL)
    assert e.value.code == STATE
    r.upload_materials(sc.materials)
    same_out(r.render(), A, "the good table again")
    qs.check(r, "the good table again")
    r.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_sky_of_another_size(api):
    from pyrtx import host
    sc = growset.materials_scene()
    r = api.Renderer(sc)
    A = r.render()
    same_out(A, reference(api, "materials", sc)["render"], "frame A")
    last = A
    for size in (32, 128, 64):
        grown = copy.copy(sc); grown.sky = host.synthetic_sky(size)
        r.upload_sky(grown.sky)
        B = r.render()
        same_out(B, reference(api, f"materials sky {size}", grown)["render"], f"a sky of {size}")
        assert differs(B, last), "rays are meant to reach the sky"
        last = B
    # rtx_update_sky goes by the size the context holds now
    new = np.ascontiguousarray(host.synthetic_sky(64)[::-1, ::-1, ::-1] * f32(0.5))
    with pytest.raises(api.RtxError):
        r.update_sky(dev(host.synthetic_sky(128)))
    t = dev(new)
    r.update_sky(t)
    grown = copy.copy(sc); grown.sky = new
    same_out(r.render(), reference(api, "materials sky updated", grown)["render"], "after rtx_update_sky of the new size")
    r.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["blas", "textures", "sky"])
def test_graph_replays_show_the_grown_state(api, monkeypatch, table):
    """RTX_GRAPH=1: warm, capture, replay before the growth; a moved table is a new graph key, so the three calls after it run eagerly,
    capture and replay again — never the graph that holds the old table's address."""
    sc = growset.materials_scene()
    keep = []
    stages = recipe(table, sc, keep)
    base = reference(api, "materials", sc)["render"]
    monkeypatch.setenv("RTX_GRAPH", "1")
    r = api.Renderer(sc)
    for i in range(3):
        same_out(r.render(serial=True), base, f"call {i} before the growth")
    for key, calls, grown in stages:
        for call in calls:
            call(r)
        want = reference(api, key, grown)["render"]
        for i in range(3):
            same_out(r.render(serial=True), want, f"{key}: call {i} after the growth")
    assert differs(want, base)
    r.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["blas", "textures", "materials", "sky"])
def test_queued_work_keeps_its_state(api, table):
    """A frame is queued, then the table grows (the call may wait; it must not change what was queued), then the next frame is rendered."""
    sc = growset.materials_scene()
    keep = []
    stages = recipe(table, sc, keep)
    before = reference(api, "materials", sc)["render"]
    r = api.Renderer(sc)
    for key, calls, grown in stages:
        r.render_async()
        for call in calls:
            call(r)
        stats, _ = r.stats()
        rgb, packed = r.framebuffer()
        same_out({"rgb": rgb, "packed": packed, "stats": stats}, before, f"{key}: the frame queued before the growth")
        before = reference(api, key, grown)["render"]
        same_out(r.render(), before, f"{key}: the frame after the growth")
    r.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_three_contexts_grow_different_tables_in_turn(api):
    sc = growset.materials_scene()
    keep = []
    tables = ("blas", "textures", "sky")
    plans = {t: recipe(t, sc, keep) for t in tables}
    ctx = {t: api.Renderer(sc) for t in tables}
    todo = {t: [call for _, calls, _ in plans[t] for call in calls] for t in tables}
    for t in tables:
        ctx[t].render_async()                                                    # every context has work queued when the others grow
    while any(todo.values()):
        for t in tables:                                                         # one step of each context in turn, nothing synchronised in between
            if todo[t]:
                todo[t].pop(0)(ctx[t])
                ctx[t].render_async()
    for t in tables:
        key, _, grown = plans[t][-1]
        same_out(ctx[t].render(), reference(api, key, grown)["render"], f"the context that grew its {t}")
    for r in ctx.values():
        r.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
def apply(r, st, keep):
    """the device calls of one edit of a growset sequence"""
    k, a = st.kind, st.args
    if k in ("blas_upload", "blas_reupload"):
        r.upload_blas(a["id"], a["blas"])
    elif k == "blas_build":
        _, idx, nrm, uv, mid = growset.source_mesh(a["name"])
        r.alloc_blas(a["id"], len(idx), len(a["positions"]), mid, a["material_offset"])
        t = (dev(a["positions"]), dev(idx, np.int32), dev(nrm), dev(uv)); keep += t
        r.build_blas(a["id"], *t)
    elif k == "blas_refit":
        if a["bind"] is not None:
            r.bind_blas_vertices(a["id"], a["bind"], len(a["positions"]))
        t = (dev(a["positions"]), dev(a["normals"])); keep += t
        r.refit_blas(a["id"], *t)
    elif k == "update_instances":
        t = (dev(a["positions"]), dev(a["rotations"])); keep += t
        r.update_instances(*t)
    elif k == "texture":
        r.alloc_texture(a["id"], a["width"], a["height"])
        t = dev(a["level0"]); keep.append(t)
        r.update_texture(a["id"], t)
    elif k in ("materials_same", "materials_more"):
        r.upload_materials(a["materials"])
    elif k == "sky":
        r.upload_sky(a["sky"])
    elif k == "masks":
        if a["how"] == "device":
            t = dev(a["masks"].view(np.int32), np.int32); keep.append(t)
            r.set_object_masks(t)
        else:
            r.set_object_masks(a["masks"])
    else:
        assert k == "set_frame"
        r.set_frame(st.scene)
        if a["drop_masks"]:
            r.set_object_masks(None)


def run_sequence(api, seed, repeats):
    r = None
    keep = []
    for k, st in enumerate(growset.sequence(seed)):
        if r is None:
            r = api.Renderer(growset.first_scene())                              # the shadow scene before the first edit
        apply(r, st, keep)
        ob = st.observe
        what = f"seed {seed} step {k}: {st.kind}, then {ob['kind']}"
        if ob["kind"] in growset.RENDERS:
            fresh = api.Renderer(st.scene)
            want = frame(fresh, api, ob["kind"], st.scene)
            fresh.close()
            if ob["kind"] == "render":
                import orc
                same_out(want, orc.OracleScene(st.scene).render(threads=8), what + " (fresh context vs oracle)")
            for i in range(repeats):
                same_out(frame(r, api, ob["kind"], st.scene), want, f"{what}, call {i}")
        else:
            want = answers(ob["kind"], st.scene, ob["rows"], ob["mask"], st.masks)
            rows_t = dev(ob["rows"])
            for i in range(repeats):
                check_answers(ob["kind"], ask(r, ob["kind"], rows_t, ob["sort"], ob["mask"]), want, f"{what}, call {i}")
    r.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_sequences_on_one_context(api, seed):
    run_sequence(api, seed, 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequences_with_graph_replay(api, monkeypatch, seed):
    monkeypatch.setenv("RTX_GRAPH", "1")
    run_sequence(api, seed, 3)
