"""Non-rigid instance matrices on the CPU (scenes and rows: tests/affineset.py):
  * the oracle against a plain float64 reference — world-space Moeller-Trumbore over the triangles moved by the float64 world matrix — on
    rays aimed into triangles of scaled, mirrored, sheared and mixed scenes: the same hit or miss, the same instance, the distance within a
    measured relative tolerance, the triangle up to float64 near-ties;
  * every class reaches the branch it is there for (zero local direction components and box-plane membership for the flattened ones, a
    negative determinant, non-zero Gram terms, NaN pixels from non-unit shading normals);
  * the safety condition of every row tests/test_gpu_affine.py sends: finite matrices with cells of at most 2^10, finite local origins and
    directions in numpy float32 in csrc/rtx_math.h's order of operations;
  * the finding that made the length queries refuse such frames, kept as a record: on the golden cube enlarged by 2 the walk twins pruned by
    a world-space box distance against a bound in local units and lost answers the exhaustive twins give; they now return RTX_ERR_STATE;
  * the rigid predicate (host.instances_rigid, the definition rtx_set_frame compiles) and the measurement behind its tau."""
import numpy as np
import pytest

import affineset as A
import util

f32, f64 = np.float32, np.float64
STATE = 5
# The largest relative gap |t_oracle - t_float64| / t_float64 per class, in units of u = 2^-24, measured on the CPU over seeds 7 .. 12 of
# A.aimed_rays, 96 rays per base scene and seed (1152 rays per class; DESIGN.md 6, Non-rigid matrices).  The large figures belong to single
# grazing rays and, for `tiny`, to materials, whose world_inv cells reach 9216.  The test runs seed 7 and carries four times the figure.
MEASURED_GAP_U = {"uniform2": 25, "uniform_half": 1764, "tiny": 1123, "nonuniform": 222, "mirror": 75, "shear": 1039, "mixed": 38}
RAYS, SEED = 96, 7
TRIANGLE_CAP = 0.05


@pytest.fixture(scope="module")
def host():
    from pyrtx import host as h
    h.lib()
    return h


# ---- the oracle against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", A.ORACLE_CLASSES)
@pytest.mark.parametrize("base", A.BASES)
def test_oracle_equals_the_float64_reference(base, cls):
    import orc
    sc = A.triangles_only(A.scene(base, cls))
    rays = A.aimed_rays(sc, RAYS, SEED)
    assert len(rays) >= 60
    tris = A.world_triangles(sc)
    t, k, runner_up = A.trace64(tris, rays)
    hits, ids = orc.OracleScene(sc).trace_closest(np.concatenate([rays, np.zeros((len(rays), 12), f32)], axis=1))
    hit = hits[:, 0] > 0
    assert np.array_equal(hit, np.isfinite(t)), f"hit or miss differs on rows {np.flatnonzero(hit != np.isfinite(t)).tolist()}"
    assert hit.sum() >= 60, int(hit.sum())                              # the rays are aimed into triangles: nearly all of them hit
    gap = np.abs(hits[hit, 1].astype(f64) - t[hit]) / t[hit]
    tol = 4 * MEASURED_GAP_U[cls] * A.U
    print(f"{base} {cls}: largest relative gap {gap.max() / A.U:.1f} u over {int(hit.sum())} hits (bound {4 * MEASURED_GAP_U[cls]} u)")
    assert gap.max() <= tol, (gap.max() / A.U, 4 * MEASURED_GAP_U[cls])
    assert np.array_equal(ids[hit, 1], tris[3][k[hit]]), "another instance"
    canon = [A.canonical_slots(sc.blas[int(b)]) for b in sc.instances["blas_id"]]
    same = np.array([canon[i][a] == canon[i][b] for i, a, b in zip(ids[hit, 1], ids[hit, 2], tris[4][k[hit]])])
    near_tie = (runner_up[hit] - t[hit]) / t[hit] <= tol
    assert np.all(same | near_tie), f"another triangle without a float64 runner-up within the tolerance: rows {np.flatnonzero(~(same | near_tie)).tolist()}"
    print(f"{base} {cls}: {int((~same).sum())} of {int(hit.sum())} rows name another triangle")
    assert (~same).sum() <= TRIANGLE_CAP * len(rays), int((~same).sum())


# ---- every class reaches its branch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", A.BASES)
def test_flattened_instances_give_zero_direction_components_and_the_plane_membership_they_name(base):
    for cls, member in (("flat_on", True), ("flat_off", False)):
        sc, rays, dist, labels, hits, ids, occ = A.ray_rows(base, cls)
        assert (hits[:, 0] > 0).sum() >= 40 and len(np.unique(ids[ids[:, 1] >= 0, 1])) >= 1
        for i in range(len(sc.instances)):
            wi = sc.instances["world_inv"][i]
            assert not np.asarray(wi, f32).reshape(4, 4)[A.FLAT_AXIS, :3].any()
            ld, lo = A.xform_dir32(wi, rays[:, 3:6]), A.xform_pos32(wi, rays[:, :3])
            assert np.all(ld[:, A.FLAT_AXIS] == 0), "every local direction has an exact zero component"
            planes = A.node_planes(sc.blas[int(sc.instances["blas_id"][i])], A.FLAT_AXIS)
            assert np.all(np.isin(lo[:, A.FLAT_AXIS], planes) == member), (cls, i)
            assert A.plane_member(sc, i) == member
            assert np.all(lo[:, A.FLAT_AXIS] != 0), "a constant of exactly 0 is not among the cases"
        frame_o, frame_d = A.camera_rows(sc)
        assert np.all(A.xform_dir32(sc.instances["world_inv"][0], frame_d)[:, A.FLAT_AXIS] == 0)


@pytest.mark.parametrize("base", A.BASES)
def test_mirror_shear_and_uniform_scale_are_what_they_are_called(base):
    import orc
    mirror, shear = A.scene(base, "mirror"), A.scene(base, "shear")
    for i in range(len(mirror.instances)):
        assert np.linalg.det(A.mat4(mirror.instances["world"][i])[:3, :3]) < 0 and np.linalg.det(A.mat4(mirror.instances["world_inv"][i])[:3, :3]) < 0
        R = A.mat4(shear.instances["world"][i])[:3, :3]
        gram = R @ R.T
        assert np.abs(gram - np.diag(np.diag(gram))).max() > 0.1, "off-diagonal Gram terms"
    mixed = A.scene(base, "mixed")
    kinds = [A.MIXED[i % len(A.MIXED)] for i in range(len(mixed.instances))]
    assert base == "cube" or (None in kinds and len(set(kinds)) == len(A.MIXED)), "a different class per instance, identity among them"
    plain = A.base_scene(base)
    for i, kind in enumerate(kinds):
        assert (mixed.instances["world"][i].tobytes() == plain.instances["world"][i].tobytes()) == (kind is None)


def test_uniform_scale_leaves_non_unit_shading_normals_and_nan_pixels_in_the_oracle():
    import orc
    ref = orc.OracleScene(A.scene("materials", "uniform2")).render(threads=4)
    assert np.isnan(ref["rgb"]).any(axis=-1).sum() > 0
    sc, rays, dist, labels, hits, ids, occ = A.ray_rows("materials", "uniform2")
    tri = (hits[:, 0] > 0) & (ids[:, 2] >= 0)
    length = np.linalg.norm(hits[tri, 5:8].astype(f64), axis=1)
    assert tri.sum() > 20 and np.all(np.abs(length - 2.0) < 1e-5), "transform_direction(world, unit normal): twice as long"


# ---- the safety condition of everything tests/test_gpu_affine.py sends ------------------------------------------------------------------------
def test_every_matrix_and_every_row_a_gpu_test_sends_is_safe():
    from test_gpu_views import camera_set
    for base in A.BASES:
        for cls in A.CLASSES:
            assert A.matrices_safe(A.scene(base, cls)) == ((base, cls) in A.GPU_SETS), (base, cls)
    assert set(A.UNSAFE) == {("materials", "tiny")} and float(np.abs(A.scene("materials", "tiny").instances["world_inv"]).max()) == 9216.0
    for base, cls in A.GPU_SETS:
        sc, rays, dist, labels, hits, ids, occ = A.ray_rows(base, cls)
        assert len(rays) <= 448
        assert A.matrices_safe(sc), (base, cls)
        assert A.rows_safe(sc, rays[:, :3], rays[:, 3:6]), (base, cls, "rays")
        assert A.rows_safe(sc, *A.camera_rows(sc)), (base, cls, "primary rays")
        # what the length queries are sent after update_instances, on mirror, and in the refusals (which queue nothing)
        points, sweeps, boxes, box_sweeps = A.length_rows(sc)
        assert A.rows_safe(sc, points[:, :3]) and A.rows_safe(sc, sweeps[:, :3], sweeps[:, 3:6]) and A.rows_safe(sc, boxes[:, :3])
        assert A.rows_safe(sc, box_sweeps[:, :3], box_sweeps[:, 3:6])
    for base in A.BASES:
        sc = A.scene(base, "mixed")
        assert A.rows_safe(sc, *A.camera_rows(sc, camera_set(sc))), (base, "views")
    # a NaN or an infinite cell is what rtx_set_frame refuses: the predicate says so for the matrices the refusal test hands over
    bad = A.scene("cube", "mirror")
    for value in (np.nan, np.inf, -np.inf):
        for field, cell in (("world", 3), ("world_inv", 7), ("world", 0)):
            b = bad.instances.copy(); b[field][0][cell] = value
            bad2 = A.scene("cube", "mirror"); bad2.instances = b
            assert not A.matrices_safe(bad2)


# ---- the finding and its fix ----------------------------------------------------------------------------------------------------------------------
def test_walk_twins_refuse_the_scaled_cube_and_the_exhaustive_twins_still_answer(host):
    """The record (A.FINDING): before the refusal host.query_nearest answered inf for (6, .1, .2) within 2.5 and (3.2, .1, .2) within .7,
    host.query_sweep inf, host.query_overlap count 0 and host.query_sweep_box inf on these rows, where the exhaustive twins give 2.0, 0.6,
    3.47, 2 and 2.40: the TLAS prune compares a world-space box distance with a bound kept in local units."""
    sc = A.finding_scene()
    assert not host.instances_rigid(sc.instances)
    rows, was, want = A.FINDING["nearest"]
    assert np.allclose(host.query_nearest_exhaustive(sc, rows)["distance"], want, rtol=1e-6)
    assert np.allclose(np.abs(host.query_signed_distance(sc, rows, exhaustive=True)["signed_distance"]), want, rtol=1e-6)
    rows_s, _, want_s = A.FINDING["sweep"]
    assert np.allclose(host.query_sweep_exhaustive(sc, rows_s)["distance"], want_s, atol=5e-3)
    rows_o, _, want_o = A.FINDING["overlap"]
    assert host.query_overlap(sc, rows_o, exhaustive=True)["count"].tolist() == list(want_o)
    assert host.query_overlapped(sc, rows_o, exhaustive=True).tolist() == [1]
    rows_b, _, want_b = A.FINDING["sweep_box"]
    assert np.allclose(host.query_sweep_box_exhaustive(sc, rows_b)["distance"], want_b, atol=5e-3)
    calls = [lambda **kw: host.query_nearest(sc, rows, **kw), lambda **kw: host.query_signed_distance(sc, rows, **kw),
             lambda **kw: host.query_sweep(sc, rows_s, **kw), lambda **kw: host.query_overlap(sc, rows_o, **kw),
             lambda **kw: host.query_overlapped(sc, rows_o, **kw), lambda **kw: host.query_sweep_box(sc, rows_b, **kw)]
    for call in calls:
        for kw in ({}, {"mask": 1}):                                      # the filtered forms refuse the same way
            with pytest.raises(ValueError, match=f"status {STATE}"):
                call(**kw)
    # t is invariant under an affine map: the segment query answers, and equals its exhaustive twin
    seg = np.array([[6, .1, .2, -1, 0, 0, 100], [6, 2.6, 0, -1, 0, 0, 100]], f32)
    walk, full = host.query_hits(sc, seg), host.query_hits_exhaustive(sc, seg)
    assert np.array_equal(walk["count"], full["count"]) and walk["count"].tolist() == [2, 0]
    assert np.array_equal(walk["distance"].view(np.uint32), full["distance"].view(np.uint32))
    # the argument checks still come first
    import ctypes as C
    s, keep = host.nearest_scene(sc)
    assert host.lib().rtxh_query_nearest(C.byref(s), None, 2, 1, None, None) == 1


@pytest.mark.parametrize("cls", A.CLASSES)
@pytest.mark.parametrize("base", A.BASES)
def test_rigid_predicate_names_the_classes(host, base, cls):
    sc = A.scene(base, cls)
    rigid, deviation = host.instances_rigid(sc.instances, deviation=True)
    assert rigid == (cls == "mirror") and (deviation > 0.5) == (cls != "mirror"), (rigid, deviation)
    points, sweeps, boxes, box_sweeps = A.length_rows(sc, 4)
    points[:, 3] = np.inf                                                  # the exhaustive search measures in local units: no maximum
    if cls == "mirror":
        walk, full = host.query_nearest(sc, points), host.query_nearest_exhaustive(sc, points)
        assert np.allclose(walk["distance"], full["distance"], rtol=1e-5)
    else:
        with pytest.raises(ValueError, match=f"status {STATE}"):
            host.query_nearest(sc, points)
        assert np.isfinite(host.query_nearest_exhaustive(sc, points)["distance"]).all()


TAU = 2.0 ** -12


def test_tau_is_four_times_what_unit_quaternions_and_the_suites_scenes_reach(host):
    """tau = 2^-12 (csrc/rtx_update_math.h RTXU_RIGID_TAU).  Measured: 7.2e-7 over 10^5 random float32 unit quaternions through
    host.instance_update (20 000 here), 4.1e-7 over the goldens, 2.8e-6 over the fuzz scenes (axes written with six decimals) and 3.9e-5 for
    many_instances, whose axes are written with five and which Quaternion::axis_angle does not normalise: the largest."""
    from pyrtx import scene_io as sio
    import sideset
    import hitset
    from test_gpu_rays import SETS, load_set
    rng = np.random.default_rng(2024)
    n = 20000
    q = sideset.random_quaternions(n, rng); p = rng.uniform(-50, 50, (n, 3)).astype(f32)
    inst = np.zeros(n, sio.INSTANCE)
    lo, hi = np.full(3, -1, f32), np.full(3, 1, f32)
    for i in range(n):
        inst[i] = host.instance_update(p[i], q[i], lo, hi, 0)[0][0]
    rigid, deviation = host.instances_rigid(inst, deviation=True)
    print(f"unit quaternions: {deviation:.3g}")
    assert rigid and deviation * 4 <= TAU and deviation < 1e-6
    worst = {}
    for name in util.GOLDENS:
        worst[name] = host.instances_rigid(util.load_golden(name)[0].instances, deviation=True)
    for name in SETS:
        worst[name] = host.instances_rigid(load_set(name).instances, deviation=True)
    worst["closed"] = host.instances_rigid(sideset.closed_scene()[0].instances, deviation=True)
    worst["rules"] = host.instances_rigid(sideset.rules_scene()[0].instances, deviation=True)
    worst["quad_stack"] = host.instances_rigid(hitset.quad_stack_scene().instances, deviation=True)
    worst["cube_pose"] = host.instances_rigid(hitset.cube_pose_scene().instances, deviation=True)
    for base in A.BASES:
        worst["affine " + base] = host.instances_rigid(A.base_scene(base).instances, deviation=True)
    print({k: f"{v[1]:.3g}" for k, v in worst.items()})
    assert all(r for r, _ in worst.values()), {k: v for k, v in worst.items() if not v[0]}
    largest = max(d for _, d in worst.values())
    assert largest * 4 <= TAU < largest * 8, (largest, TAU)             # the power of two at least four times the measurement
    assert worst["many_instances"][1] == largest
    # the edge of the predicate itself, in float64 on float32 cells: a scale of 1 + e has R.R^T - I = 2e + e^2 on the diagonal
    one = util.load_golden("cube")[0].instances[:1].copy()
    for e, want in ((2.0 ** -14, True), (2.0 ** -12, False)):
        m = one.copy()
        m["world"][0][[0, 5, 10]] = f32(1 + e)
        assert host.instances_rigid(m) == want, e
    m = one.copy(); m["world_inv"][0][1] = f32(2.0 ** -11)
    assert not host.instances_rigid(m), "world_inv is judged too"
    m = one.copy(); m["world"][0][5] = np.nan
    assert not host.instances_rigid(m) and np.isnan(host.instances_rigid(m, deviation=True)[1])
    assert host.instances_rigid(one[:0]), "no instances: rigid"
