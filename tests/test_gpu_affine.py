"""Scaled, mirrored, sheared, mixed and flattened instance matrices through every kernel that reads an instance (scenes and rows:
tests/affineset.py; each matrix and each row is checked for safety on the CPU first, tests/test_affine_cpu.py), bit for bit (NaN == NaN)
against the oracle:
  * frames in every launch shape of test_gpu_parity.MODES: colours, packed pixels, the four ray counts, and no stack overflow reported;
  * the adversarial rows of tests/rayset.py through rtx_debug_trace_rays, rtx_debug_occluded, rtx_query_closest and rtx_query_occluded under
    every kernel flag, sorted and unsorted, and rtx_query_hits against its host twin;
  * on the mixed scene: a batch of views, an AOV call (normals are the non-unit ones the oracle stores), caller-supplied pinhole rays, the
    group loopback at world 3;
  * the length queries (nearest, signed distance, sweep, overlap, overlapped, sweep box, filtered forms included) refuse a frame with a
    non-rigid instance with RTX_ERR_STATE and queue nothing; a reflection is accepted and equals the twins; after rtx_update_instances with
    unit quaternions they answer again; rtx_set_frame refuses a NaN or infinite matrix cell and keeps the previous frame.
No test here sends a matrix with a non-finite cell past rtx_set_frame."""
import copy

import numpy as np
import pytest

import affineset as A
import util
from test_gpu_parity import MODES
from test_gpu_query import FLAGS, check_channels, dev, expected, host as to_host, same_bits, segments_of
from test_gpu_rays import LANE_TRACE, PACKET_CLOSEST, check_occ, occluded

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, STATE = 1, 5
SET_IDS = [f"{b}-{c}" for b, c in A.GPU_SETS]
ALL = ("distance", "position", "normal", "uv", "material_id", "object_id", "triangle_id")
_ORACLE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def oracle_frame(base, cls):
    if (base, cls) not in _ORACLE:
        import orc
        _ORACLE[base, cls] = orc.OracleScene(A.scene(base, cls)).render(threads=8)
    return _ORACLE[base, cls]


def assert_frame(out, ref, what):
    assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])
    assert util.bit_exact(out["rgb"], ref["rgb"]), f"{what}: rgb differs on {int((~same_bits(out['rgb'].reshape(-1, 3), ref['rgb'].reshape(-1, 3))).sum())} pixels"
    assert np.array_equal(out["packed"], ref["packed"]), what


def read_back(r, sc):
    inst, nodes, idx = r.read_frame_state()
    return (inst, nodes, idx, sc.spheres, sc.planes), [r.read_blas(b) for b in range(len(sc.blas))]


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,cls", A.GPU_SETS, ids=SET_IDS)
def test_frames_equal_the_oracle_in_every_launch_shape(api, base, cls):
    sc = A.scene(base, cls)
    ref = oracle_frame(base, cls)
    assert ref["stats"]["primary"] == A.WIDTH * A.HEIGHT
    r = api.Renderer(sc)
    for mode, kw in MODES.items():
        assert_frame(r.render(**kw), ref, f"{base} {cls} {mode}")      # render() reads the stats: a stack overflow would raise RTX_ERR_LIMIT there
    r.close()


# ---- rays -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,cls", A.GPU_SETS, ids=SET_IDS)
def test_ray_rows_equal_the_oracle_through_every_kernel(api, base, cls):
    import orc
    import rayset
    from pyrtx import host
    sc, rays, dist, labels, hits, ids, occ = A.ray_rows(base, cls)
    assert len(rays) <= 448
    assert A.RAY_CLASSES[:-1] == rayset.CLASSES
    classes = np.array(A.RAY_CLASSES); lab = np.array([list(classes).index(x) for x in labels])
    r = api.Renderer(sc)
    for flags in (0, LANE_TRACE, PACKET_CLOSEST):
        util.check_hits(r.debug_trace_rays(rays, flags), hits, lab, classes)
    for flags in (0, LANE_TRACE):
        check_occ(occluded(r, rays, dist, flags), occ, labels)
    rays6 = np.ascontiguousarray(rays[:, :6])
    want = expected(orc.OracleScene(sc), rays6)
    rays_t, seg_t = dev(rays6), dev(segments_of(rays6, dist))
    for sort in (False, True):
        for flags, kw in FLAGS.items():
            check_channels(r.query_closest(rays_t, tuple(api.QUERY_CHANNELS), sort=sort, **kw), want, labels, f"{base} {cls} flags {flags} sort {sort}")
            got = to_host(r.query_occluded(seg_t, sort=sort, **kw))
            check_occ(got.reshape(dist.shape) != 0, occ, labels)
    # all hits: t is invariant under an affine map, so this walk query answers on every class; against its host twin
    D = np.where(np.arange(len(rays6)) % 2 == 0, np.inf, dist[:, 2]).astype(f32)
    seg = np.ascontiguousarray(np.concatenate([rays6, D[:, None]], axis=1))
    twin = host.query_hits(sc, seg, 8, ALL)
    twin.pop("stack_max")
    for sort in (False, True):
        got = {k: to_host(v) for k, v in r.query_hits(dev(seg), 8, ALL, sort=sort).items()}
        bad = {k: int((~same_bits(got[k], twin[k])).sum()) for k in twin if not same_bits(got[k], twin[k]).all()}
        assert not bad, (base, cls, sort, bad)
    only = to_host(r.query_hits(dev(seg), 0, ())["count"])
    assert np.array_equal(only, twin["count"]) and (only > 0).sum() > 20
    mask = np.where(np.arange(len(seg)) % 3 == 0, 0, 1).astype(np.int32)
    masked = host.query_hits(sc, seg, 8, ("distance", "object_id"), mask=mask)
    got = r.query_hits(dev(seg), 8, ("distance", "object_id"), mask=dev(mask))
    assert same_bits(to_host(got["distance"]), masked["distance"]).all() and np.array_equal(to_host(got["count"]), masked["count"])
    assert not masked["count"][::3].any()
    r.close()


# ---- the mixed scene through the other render entry points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("base", A.BASES)
def test_mixed_views_equal_the_oracle(api, base):
    import orc
    from test_gpu_views import camera_set, with_camera
    sc = A.scene(base, "mixed")
    cams = camera_set(sc)
    r = api.Renderer(sc)
    r.set_views(cams)
    out = r.render_views()
    for k in range(len(cams)):
        ref = orc.OracleScene(with_camera(sc, cams[k])).render(threads=8)
        assert util.bit_exact(out["rgb"][k], ref["rgb"]) and np.array_equal(out["packed"][k], ref["packed"]), k
    r.close()


@pytest.mark.parametrize("base", A.BASES)
def test_mixed_aovs_equal_the_oracle(api, base):
    from test_gpu_aov import ALL as AOVS, IDS, flat, oracle
    from test_gpu_ray_views import assert_same
    sc = A.scene(base, "mixed")
    out = api.Renderer(sc).render_aovs(AOVS)
    dist, rays, hits, albedo, ids = oracle(f"affine {base} mixed", sc)
    assert_frame(out, oracle_frame(base, "mixed"), "the AOV call's colours")
    assert_same(flat(out, "depth"), dist, "depth")
    hit = hits[:, 0] > 0
    tri = hit & (ids[:, 2] >= 0)
    assert tri.sum() > 50
    assert_same(flat(out, "position")[hit], hits[hit, 2:5], "position")
    assert_same(flat(out, "normal")[hit], hits[hit, 5:8], "normal")
    length = np.linalg.norm(flat(out, "normal")[tri].astype(np.float64), axis=1)
    assert (np.abs(length - 1) > 0.05).any(), "the scaled instances' normals stay non-unit, as the oracle stores them"
    assert_same(flat(out, "uv")[hit], hits[hit, 9:11], "uv")
    assert_same(flat(out, "albedo"), albedo, "albedo")
    for k, ch in enumerate(IDS):
        assert_same(flat(out, ch), ids[:, k], ch)


@pytest.mark.parametrize("base", A.BASES)
def test_mixed_pinhole_rays_and_group_loopback(api, base):
    sc = A.scene(base, "mixed")
    ref = oracle_frame(base, "mixed")
    r = api.Renderer(sc)
    r.set_rays(api.pinhole_rays(sc.camera[0], sc.width, sc.height))
    out = r.render_rays()
    assert out["stats"] == ref["stats"]
    assert util.bit_exact(out["rgb"][0], ref["rgb"]) and np.array_equal(out["packed"][0], ref["packed"])
    r2 = api.Renderer(sc)
    r2.group_loopback(3)
    _, packed = r2.framebuffer()
    assert np.array_equal(packed, ref["packed"])
    r.close(); r2.close()


# ---- the length queries ---------------------------------------------------------------------------------------------------------------------------
def length_calls(r, sc, filtered):
    """name -> a call of one length query on the context, over A.length_rows(sc)."""
    points, sweeps, boxes, box_sweeps = (dev(x) for x in A.length_rows(sc))
    kw = {"mask": 1} if filtered else {}
    return {"nearest": lambda: r.query_nearest(points, ALL, **kw), "signed_distance": lambda: r.query_signed_distance(points, ALL, feature=True, **kw),
            "sweep": lambda: r.query_sweep(sweeps, ALL, **kw), "overlap": lambda: r.query_overlap(boxes, 8, **kw),
            "overlapped": lambda: {"count": r.query_overlapped(boxes, **kw)},
            "sweep_box": lambda: r.query_sweep_box(box_sweeps, ("distance", "normal", "object_id", "triangle_id", "axis"), **kw)}


def length_twins(state, blas, sc, filtered):
    from pyrtx import host
    points, sweeps, boxes, box_sweeps = A.length_rows(sc)
    kw = {"mask": 1} if filtered else {}
    out = {"nearest": host.query_nearest(state, points, ALL, blas=blas, **kw), "signed_distance": host.query_signed_distance(state, points, ALL, blas=blas, **kw),
           "sweep": host.query_sweep(state, sweeps, ALL, blas=blas, **kw), "overlap": host.query_overlap(state, boxes, 8, blas=blas, **kw),
           "overlapped": {"count": host.query_overlapped(state, boxes, blas=blas, **kw)},
           "sweep_box": host.query_sweep_box(state, box_sweeps, ("distance", "normal", "object_id", "triangle_id", "axis"), blas=blas, **kw)}
    for v in out.values():
        v.pop("stack_max", None)
    return out


def assert_answers(calls, twins, what):
    for name, call in calls.items():
        got = {k: to_host(v) for k, v in call().items()}
        assert set(got) == set(twins[name]), (what, name, set(got), set(twins[name]))
        bad = {k: int((~same_bits(got[k], twins[name][k])).sum()) for k in got if not same_bits(got[k], twins[name][k]).all()}
        assert not bad, (what, name, bad)


@pytest.mark.parametrize("base,cls", [s for s in A.GPU_SETS if s[1] in A.NONRIGID], ids=[i for i, s in zip(SET_IDS, A.GPU_SETS) if s[1] in A.NONRIGID])
def test_length_queries_refuse_a_non_rigid_frame_and_queue_nothing(api, base, cls):
    import orc
    sc = A.scene(base, cls)
    ref = oracle_frame(base, cls)
    r = api.Renderer(sc)
    r.render_async()                                                    # a frame queued before the refusals
    for filtered in (False, True):
        for name, call in length_calls(r, sc, filtered).items():
            with pytest.raises(api.RtxError) as e:
                call()
            assert e.value.code == STATE and "rigid" in str(e.value), (name, filtered, str(e.value))
    stats, _ = r.stats()
    rgb, packed = r.framebuffer()
    assert stats == ref["stats"] and util.bit_exact(rgb, ref["rgb"]) and np.array_equal(packed, ref["packed"]), "a refusal touched the queued frame"
    sc_r, rays, dist, labels, hits, ids, occ = A.ray_rows(base, cls)
    rays6 = np.ascontiguousarray(rays[:64, :6])
    check_channels(r.query_closest(dev(rays6), tuple(api.QUERY_CHANNELS)), expected(orc.OracleScene(sc), rays6), labels[:64], "a valid query after the refusals")
    r.close()


@pytest.mark.parametrize("base", A.BASES)
def test_a_reflection_is_accepted_and_equals_the_twins(api, base):
    sc = A.scene(base, "mirror")
    r = api.Renderer(sc)
    state, blas = read_back(r, sc)
    for filtered in (False, True):
        twins = length_twins(state, blas, sc, filtered)
        assert np.isfinite(twins["nearest"]["distance"]).sum() > 8
        assert_answers(length_calls(r, sc, filtered), twins, f"{base} mirror filtered {filtered}")
    r.close()


@pytest.mark.parametrize("cls", ["nonuniform", "mixed", "flat_on"])
@pytest.mark.parametrize("base", A.BASES)
def test_after_update_instances_the_length_queries_answer(api, base, cls):
    from pyrtx import host
    from test_gpu_update_instances import with_state
    sc = A.scene(base, cls)
    r = api.Renderer(sc)
    n = len(sc.instances)
    rng = np.random.default_rng(17)
    pos = np.ascontiguousarray(sc.instances["world"].reshape(n, 4, 4)[:, :3, 3] + rng.uniform(-0.25, 0.25, (n, 3))).astype(f32)
    q = rng.normal(size=(n, 4)); rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    with pytest.raises(api.RtxError):
        r.query_nearest(dev(A.length_rows(sc)[0]))
    p_t, q_t = dev(pos), dev(rot)
    r.update_instances(p_t, q_t)
    moved = with_state(sc, r.read_frame_state())
    assert host.instances_rigid(moved.instances) and A.matrices_safe(moved)
    rows = A.length_rows(moved)
    assert A.rows_safe(moved, rows[0][:, :3]) and A.rows_safe(moved, rows[1][:, :3], rows[1][:, 3:6]) and A.rows_safe(moved, rows[3][:, :3], rows[3][:, 3:6])
    state, blas = read_back(r, sc)
    twins = length_twins(state, blas, moved, False)
    assert np.isfinite(twins["nearest"]["distance"]).sum() > 8
    assert_answers(length_calls(r, moved, False), twins, f"{base} {cls} after update_instances")
    r.set_frame(sc)                                                     # the matrices as given again: refused again
    with pytest.raises(api.RtxError) as e:
        r.query_nearest(dev(rows[0]))
    assert e.value.code == STATE
    r.close()


def test_set_frame_refuses_a_non_finite_cell_and_keeps_the_previous_frame(api):
    sc = A.scene("materials", "mirror")
    ref = oracle_frame("materials", "mirror")
    r = api.Renderer(sc)
    assert_frame(r.render(), ref, "before")
    for value in (np.nan, np.inf, -np.inf):
        for field, i, cell in (("world", 0, 3), ("world_inv", len(sc.instances) - 1, 7), ("world", 1, 0), ("world_inv", 2, 10)):
            bad = copy.deepcopy(sc)
            inst = bad.instances.copy(); inst[field][i][cell] = value
            bad.instances = inst
            bad.camera = bad.camera.copy(); bad.camera["position"] += f32(1.0)      # a frame that would look different
            with pytest.raises(api.RtxError) as e:
                r.set_frame(bad)
            assert e.value.code == INVALID and "NaN or infinite" in str(e.value), (value, field, str(e.value))
    assert_frame(r.render(), ref, "after the refused frames")
    state, blas = read_back(r, sc)
    assert state[0].tobytes() == sc.instances.tobytes()
    assert_answers({"nearest": length_calls(r, sc, False)["nearest"]}, length_twins(state, blas, sc, False), "the length queries still see the mirrored frame")
    r.close()
