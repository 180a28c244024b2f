"""Signed-distance queries without a GPU (include/rtx.h: rtx_blas_pseudonormals / rtx_query_signed_distance; the host twins
rtxh_blas_pseudonormals / rtxh_query_signed_distance, which run csrc/rtx_side_math.h, the code the kernels compile).

  tables     the twin against a numpy float64 restatement on the golden meshes: the angle between each record and its float64 record is at
             most DELTA = 4 x the largest deviation measured on these meshes (sideset.MEASURED_DEVIATION = 9.19e-7 rad -> 3.68e-6 rad); the
             structural cases are exact (bit for bit);
  sign       against an independent oracle, the float64 generalized winding number of the posed triangles (inside iff |w| > 0.5): the five
             closed meshes posed by random unit quaternions, one mirrored; 2000 uniform rows in 1.25 x the world box and rows offset to both
             sides of every edge midpoint and vertex of Rock and Diamond by 1e-3 of the mesh size.  A row is left out when its float64
             distance is at most rtxh_nearest_distance_bound(S, W) or the float64 |cos(r, N)| is at most bound / |r| + DELTA; at most 2 % may
             be left out; every kept row has the oracle's sign.  60 points exactly on faces, edges and vertices of the posed meshes are among
             the rows: posed, they are on the surface only to rounding, and must be left out or come back + 0 (exact + 0: the unposed Cube).  The same rows without tables (feature + 8) disagree with the oracle on Rock;
  open       sheets: above and below, beyond the boundary, on both sides of a fold; Monkey's face-region rows against the float64 face normal;
  rules      spheres, planes, dead rows, mask 0, distance == |signed| bit for bit, walk == exhaustive wherever they return one primitive.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import normalset as ns
import sideset as ss
import util
from test_views_cpu import _offline_renderer

REPO = util.REPO
f32, f64 = np.float32, np.float64
NEW = ("rtx_blas_pseudonormals", "rtx_read_blas_pseudonormals", "rtx_query_signed_distance")
NEW_HOST = ("rtxh_blas_pseudonormals", "rtxh_query_signed_distance", "rtxh_query_signed_distance_filtered", "rtxh_query_signed_distance_exhaustive",
            "rtxh_query_signed_distance_exhaustive_filtered")


@pytest.fixture(scope="module")
def host():
    from pyrtx import host as h
    h.lib()
    return h


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.ascontiguousarray(a, f32).tobytes() == np.ascontiguousarray(b, f32).tobytes()


def test_functions_are_declared_exported_and_bound(host):
    from pyrtx import api
    header = open(f"{REPO}/include/rtx.h").read()
    lib = api.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"\sT\s+" + name + r"\b", exported), f"{name} is not exported by the library"
        assert name in api.EXPORTS and name in api.SIGNED_EXPORTS, name
        assert getattr(lib, name).argtypes and getattr(lib, name).restype is C.c_int, name
    host_header = open(f"{REPO}/include/rtx_host.h").read()
    hlib = host.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", hlib._name], capture_output=True, text=True, check=True).stdout
    for name in NEW_HOST:
        assert re.search(r"\bint\s+" + name + r"\s*\(", host_header), name
        assert re.search(r"\sT\s+" + name + r"\b", exported), name
        assert name in host.EXPORTS and getattr(hlib, name).argtypes, name
    assert "Out of scope: signed distance" not in header
    assert "rtx_query_signed_distance" in header[header.index("all-hits segment queries"):header.index("int rtx_query_hits(")]


def test_side_check_program():
    """The device plan on the CPU against the plain loop, and triangle_region against triangle_d2, under the host sanitizers."""
    out = subprocess.run(["make", "-B", "-C", os.path.join(REPO, "cpu-raytracer_amd", "csrc"), "side_check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "side_check: ok" in out.stdout


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", list(ss.CLOSED) + ["Monkey"])
def test_tables_against_the_float64_restatement(host, mesh):
    """Largest angle measured: Cube 0, Diamond 1.02e-7, Rock 1.35e-7, Torus 1.02e-7, icosphere 1.07e-7, Monkey 9.19e-7 rad (a vertex whose
    corner vectors nearly cancel).  Allowed: DELTA = 4 x 9.19e-7.  Records whose float64 length is below 1e-3 (Monkey: one vertex, four
    edge records of coincident opposite faces) have no direction; the twin's are as short."""
    pos, idx, blas, sv = ss.golden_mesh(mesh)
    vert, edge = host.blas_pseudonormals(pos, idx, sv)
    assert vert.shape == (len(pos), 4) and edge.shape == (len(sv), 3, 4) and vert.dtype == f32 and edge.dtype == f32
    assert np.isfinite(vert).all() and np.isfinite(edge).all()
    assert (bits(vert[:, 3]) == 0).all() and (bits(edge[:, :, 3]) == 0).all()
    v64, e64, _ = ss.tables64(pos, idx, sv)
    worst = 0.0
    for got, want in ((vert[:, :3], v64), (edge[:, :, :3].reshape(-1, 3), e64.reshape(-1, 3))):
        big = np.linalg.norm(want, axis=1) > 1e-3
        worst = max(worst, float(ss.angle_between(got[big], want[big]).max()))
        assert (np.linalg.norm(got[~big].astype(f64), axis=1) < 2e-3).all()
        assert np.abs(np.linalg.norm(got[big].astype(f64), axis=1) / np.linalg.norm(want[big], axis=1) - 1).max() < 1e-5
    print(f"{mesh}: largest angle between the twin and float64 {worst:.3e} rad (allowed {ss.DELTA:.3e})")
    assert worst <= ss.DELTA, (mesh, worst)


def np_unit_normal(p0, p1, p2):
    """FACE of rtx_side_math.h in numpy float32."""
    e1, e2 = p1 - p0, p2 - p0
    f = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
    m = np.abs(f).max()
    a = f / m
    return a / np.sqrt(a[0] * a[0] + (a[1] * a[1] + a[2] * a[2]))


def test_structural_cases_are_exact(host):
    pos = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.7, 0.6], [9, 9, 9]], f32)
    idx = np.array([[0, 1, 2]], np.int32)
    vert, edge = host.blas_pseudonormals(pos, idx, idx)
    n = np_unit_normal(pos[0], pos[1], pos[2])
    for k in range(3):
        assert same(edge[0, k, :3], n), "a boundary edge equals the unit face normal bit for bit"
    assert (bits(vert[3]) == 0).all(), "an unused vertex gives zero"
    assert abs(float(np.linalg.norm(vert[:3, :3].astype(f64).sum(0))) - np.pi) < 1e-5, "the three corner angles of a triangle"
    # two coincident opposite faces
    vert, edge = host.blas_pseudonormals(pos, np.array([[0, 1, 2], [0, 2, 1]], np.int32), np.array([[0, 1, 2], [0, 2, 1]], np.int32))
    assert (vert == 0).all() and (edge == 0).all()
    # pad slots, pad triangles
    pos, idx = ns.indexed("icosphere")
    sv = np.concatenate([idx, [[-1, -1, -1]], idx[:2]]).astype(np.int32)
    clean_v, clean_e = host.blas_pseudonormals(pos, idx, idx)
    vert, edge = host.blas_pseudonormals(pos, ns.padded(idx, len(pos)), sv)
    assert same(vert, clean_v) and same(edge[:len(idx)], clean_e), "invalid triangles contribute nothing"
    assert (bits(edge[len(idx)]) == 0).all(), "a pad slot gives zero"
    assert same(edge[len(idx) + 1:], clean_e[:2]), "repeated slots give equal records"
    # a non-manifold edge gets the sum of all its faces, whichever slot asks and in whichever direction
    pos = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.3, 1], [0.5, -1, -0.4]], f32)
    idx = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32)
    vert, edge = host.blas_pseudonormals(pos, idx, idx)
    want = np.zeros(3, f32)
    for t in idx:
        want = want + np_unit_normal(*pos[t])
    assert same(edge[0, 0, :3], want) and same(edge[1, 0, :3], want) and same(edge[2, 0, :3], want)


def test_repeated_slots_of_an_sbvh_get_their_twins_records(host):
    pos, idx, blas, sv = ss.golden_mesh("Monkey", True)
    assert len(sv) > len(idx), "the SBVH tree is meant to hold duplicated references"
    vert, edge = host.blas_pseudonormals(pos, idx, sv)
    first = {}
    for s, t in enumerate(blas.order):
        if int(t) in first:
            assert same(edge[s], edge[first[int(t)]])
        first.setdefault(int(t), s)
    assert len(first) == len(idx)


# ---- the sign against the winding number ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def closed_case(host):
    sc, meshes = ss.closed_scene()
    rng = np.random.default_rng(5)
    uniform = ss.uniform_rows(sc, meshes, 2000, rng)
    feature = ss.feature_rows(sc, meshes, (1, 2))
    surface = ss.surface_rows(sc, meshes, 10, rng)                    # 60 rows: with them the cap of 2 % still holds
    pts = np.concatenate([uniform, feature, surface])
    rows = ss.as_rows(pts)
    tris, owner = ss.posed_triangles(sc, meshes)
    inside = np.abs(ss.winding_number(rows[:, :3], tris)) > 0.5
    left_out, dist64 = ss.undetermined(sc, meshes, rows)
    with_tables = host.query_signed_distance(sc, rows, channels=("distance", "object_id", "triangle_id"), pseudonormals=ss.host_tables(meshes))
    naive = host.query_signed_distance(sc, rows, channels=("object_id",))
    return dict(sc=sc, meshes=meshes, rows=rows, inside=inside, left_out=left_out, dist64=dist64, got=with_tables, naive=naive, n_uniform=len(uniform), n_surface=len(surface))


def test_sign_against_the_winding_number(closed_case):
    c = closed_case
    got, keep = c["got"], ~c["left_out"]
    print(f"{len(keep)} rows, {int(c['left_out'].sum())} left out ({100 * c['left_out'].mean():.3f} %), {int(c['inside'].sum())} inside, "
          f"nearest uniform row at {c['dist64'][:c['n_uniform']].min():.3e}; features met: {np.bincount(got['feature'], minlength=4)[1:4]}")
    assert c["left_out"].mean() <= 0.02
    assert c["inside"][:c["n_uniform"]].sum() > 20 and (~c["inside"][:c["n_uniform"]]).sum() > 20
    assert (got["feature"] >= 1).all() and (got["feature"] <= 3).all()
    assert set(np.unique(got["feature"])) == {1, 2, 3}, "faces, edges and vertices all decide rows"
    assert set(np.unique(got["object_id"])) == set(range(len(c["meshes"]))), "every instance, the mirrored one included, owns rows"
    wrong = keep & ((got["signed_distance"] < 0) != c["inside"])
    assert not wrong.any(), (np.nonzero(wrong)[0][:10], got["feature"][wrong][:10], got["object_id"][wrong][:10])
    assert same(np.abs(got["signed_distance"]), got["distance"])


def test_posed_points_on_the_surface_are_left_out_or_plus_zero(closed_case):
    """Points exactly on faces, edges and vertices of the posed meshes (60 rows).  A posed point is on the surface only to the rounding of its
    float32 coordinates and of the instance's matrix, so its sign is not determined: every such row must fall under the leave-out rule (its
    float64 distance within rtxh_nearest_distance_bound) or come back + 0, and its distance must be of that size.  The exact + 0 is pinned
    where the points are exact: test_points_on_the_surface_give_plus_zero."""
    c = closed_case
    k = c["n_surface"]
    sd, out, d64 = c["got"]["signed_distance"][-k:], c["left_out"][-k:], c["dist64"][-k:]
    zero = bits(sd) == 0
    print(f"{k} posed on-surface rows: {int(out.sum())} left out, {int(zero.sum())} + 0, largest |signed| {np.abs(sd).max():.3e}, largest float64 distance {d64.max():.3e}")
    assert (out | zero).all()
    assert not (c["left_out"][:-k]).any(), "no other row is left out: the cap is spent on these"
    assert np.abs(sd).max() < 4e-5, "rtxh_nearest_distance_bound(S, W) for S <= 8, W <= 40 in this scene is 3.6e-5"
    assert set(np.unique(c["got"]["feature"][-k:])) <= {1, 2, 3}


def test_the_naive_rule_is_told_apart_on_rock(closed_case):
    c = closed_case
    naive, keep = c["naive"], ~c["left_out"]
    assert (naive["feature"] >= 9).all() and (naive["feature"] <= 11).all()
    assert same(np.abs(naive["signed_distance"]), np.abs(c["got"]["signed_distance"]))
    rock = np.isin(naive["object_id"], (2, 5))
    wrong = keep & rock & ((naive["signed_distance"] < 0) != c["inside"])
    print(f"the face rule alone is wrong on {int(wrong.sum())} of {int((keep & rock).sum())} kept rows of Rock")
    assert wrong.sum() >= 1
    face = c["got"]["feature"] == 1
    assert (np.signbit(naive["signed_distance"][face]) == np.signbit(c["got"]["signed_distance"][face])).all(), "in a face region the two rules are one"


def test_points_on_the_surface_give_plus_zero(host):
    """Cube at the identity: its vertices, edge midpoints and face centres are exact in float32."""
    meshes = [ss.golden_mesh("Cube")]
    sc = ss.posed_scene(meshes, np.zeros((1, 3), f32), np.array([[0, 0, 0, 1]], f32))
    pos, idx = meshes[0][0].astype(f64), meshes[0][1]
    tri = pos[idx]
    pts = np.concatenate([pos, (tri[:, 0] + tri[:, 1]) / 2, (tri[:, 1] + tri[:, 2]) / 2, (tri[:, 0] + tri[:, 2]) / 2, (tri[:, 0] + tri[:, 1] + 2 * tri[:, 2]) / 4])
    assert (pts.astype(f32).astype(f64) == pts).all()
    got = host.query_signed_distance(sc, ss.as_rows(pts), pseudonormals=ss.host_tables(meshes))
    assert (bits(got["signed_distance"]) == 0).all(), "+0, never -0"
    assert set(np.unique(got["feature"])) <= {1, 2, 3}


# ---- open surfaces ---------------------------------------------------------------------------------------------------------------------------
def sheet_scene(pos, idx):
    meshes = [(pos, idx) + ss.mesh_blas(pos, idx)]
    return ss.posed_scene(meshes, np.zeros((1, 3), f32), np.array([[0, 0, 0, 1]], f32)), meshes


@pytest.mark.parametrize("n", [1, 4])
def test_flat_sheets_above_and_below(host, n):
    """The quad (n = 1) and the 4 x 4 grid: above is +, below is -, over the sheet and beyond its boundary, where the nearest feature is a
    boundary edge or a corner vertex."""
    pos, idx = ss.sheet(n)
    sc, meshes = sheet_scene(pos, idx)
    rng = np.random.default_rng(3)
    xz = rng.uniform(-0.75 * n, 1.75 * n, (400, 2))
    y = rng.uniform(0.05, 1.0, 400) * np.where(np.arange(400) % 2, -1, 1)
    pts = np.stack([xz[:, 0], y, xz[:, 1]], 1)
    got = host.query_signed_distance(sc, ss.as_rows(pts), pseudonormals=ss.host_tables(meshes))
    assert ((got["signed_distance"] < 0) == (y < 0)).all()
    outside = (xz.min(1) < 0) | (xz.max(1) > n)
    corner = ((xz[:, 0] < 0) | (xz[:, 0] > n)) & ((xz[:, 1] < 0) | (xz[:, 1] > n))
    assert (got["feature"][outside] >= 2).all() and (got["feature"][corner] == 3).all() and (got["feature"][~outside] == 1).sum() > 20
    naive = host.query_signed_distance(sc, ss.as_rows(pts))
    assert ((naive["signed_distance"] < 0) == (y < 0)).all(), "a flat sheet has one normal: the naive rule agrees here"


@pytest.mark.parametrize("fold", [0.9, -0.9])
def test_folded_sheet_in_the_folds_edge_region(host, fold):
    """A 4 x 4 grid folded along its middle row by +-0.9 rad.  Rows on the bisecting plane of the fold, on both sides of the sheet: on the
    convex side the nearest feature is the fold's edge (or one of its vertices) and the sign must be that side's; on the concave side the
    nearest feature is a face.  `upper` is the side the +y normals of the flat half point to."""
    pos, idx = ss.sheet(4, fold)
    sc, meshes = sheet_scene(pos, idx)
    rng = np.random.default_rng(4)
    x = rng.uniform(0.2, 3.8, 200)
    h = rng.uniform(0.05, 0.6, 200) * np.where(np.arange(200) % 2, -1, 1)      # along the bisector: + is the upper side
    bis = np.array([0.0, np.cos(fold / 2), -np.sin(fold / 2)])                   # halves the angle between the two halves' normals
    pts = np.stack([x, np.zeros(200), np.full(200, 2.0)], 1) + h[:, None] * bis[None, :]
    got = host.query_signed_distance(sc, ss.as_rows(pts), pseudonormals=ss.host_tables(meshes))
    assert ((got["signed_distance"] < 0) == (h < 0)).all()
    convex_side = (h < 0) if fold > 0 else (h > 0)
    assert (got["feature"][convex_side] >= 2).all() and (got["feature"][~convex_side] == 1).all()


def test_monkey_face_regions_have_the_face_normals_sign(host):
    """Monkey is open (28 boundary edges): there is no inside.  Rows whose region is a face have the sign of the float64 face normal."""
    pos, idx, blas, sv = ss.golden_mesh("Monkey")
    meshes = [(pos, idx, blas, sv)]
    sc = ss.posed_scene(meshes, np.zeros((1, 3), f32), np.array([[0, 0, 0, 1]], f32))
    rng = np.random.default_rng(6)
    p64 = pos.astype(f64)
    c, h = (p64.min(0) + p64.max(0)) / 2, (p64.max(0) - p64.min(0)) / 2 * 1.25
    rows = ss.as_rows(rng.uniform(c - h, c + h, (1500, 3)))
    got = host.query_signed_distance(sc, rows, channels=("triangle_id", "position"), pseudonormals=ss.host_tables(meshes))
    face = got["feature"] == 1
    assert face.sum() > 300
    tri = p64[idx[blas.order[got["triangle_id"][face]]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    side = ((rows[face, :3].astype(f64) - got["position"][face].astype(f64)) * n).sum(1)
    clear = np.abs(side) > 1e-5 * np.linalg.norm(n, axis=1) * np.abs(got["signed_distance"][face])
    assert clear.mean() > 0.99
    assert ((got["signed_distance"][face] < 0) == (side < 0))[clear].all()


# ---- rules -----------------------------------------------------------------------------------------------------------------------------------
rules_scene = ss.rules_scene


def test_spheres_planes_and_dead_rows(host):
    sc, meshes = rules_scene()
    tables = ss.host_tables(meshes)
    rows = np.array([[4, 0.1, 0, np.inf], [4, 0.9, 0, np.inf], [4, 0, 0, np.inf],           # sphere 0: inside, outside, at the centre
                     [-4, 1, 1.0, np.inf], [-4, 1, 3.0, np.inf],                              # sphere 1: inside, outside
                     [9, -2.5, 9, np.inf], [9, -3.5, 9, np.inf], [9, -3, 9, np.inf],          # the plane: above, below, on it
                     [np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, 0, 0], [0, 0, 0, -1], [0, 0, 0, np.nan], [50, 50, 50, 0.5]], f32)
    got = host.query_signed_distance(sc, rows, channels=("distance", "object_id"), pseudonormals=tables)
    sd, ft = got["signed_distance"], got["feature"]
    assert list(ft[:8]) == [4, 4, 4, 4, 4, 5, 5, 5]
    assert list(np.sign(sd[:8])) == [-1, 1, -1, -1, 1, 1, -1, 0] and bits(sd[7]) == 0
    assert sd[2] == -f32(np.sqrt(f32(0.49))) and abs(sd[0] + 0.6) < 1e-6 and abs(sd[5] - 0.5) < 1e-6
    assert (ft[8:] == 0).all() and np.isposinf(sd[8:]).all() and (got["object_id"][8:] == -1).all()
    assert same(np.abs(sd), got["distance"])
    # no channel at all: the two outputs alone, the same bits
    alone = host.query_signed_distance(sc, rows, pseudonormals=tables)
    assert set(alone) == {"signed_distance", "feature", "stack_max"} and same(alone["signed_distance"], sd) and (alone["feature"] == ft).all()
    assert "feature" not in host.query_signed_distance(sc, rows, pseudonormals=tables, feature=False)


def test_masks_and_the_exhaustive_twin(host):
    sc, meshes = rules_scene()
    tables = ss.host_tables(meshes)
    rng = np.random.default_rng(9)
    rows = ss.as_rows(rng.uniform(-5, 5, (600, 3)), 6.0)
    names = ("distance", "position", "normal", "uv", "material_id", "object_id", "triangle_id")
    walk = host.query_signed_distance(sc, rows, channels=names, pseudonormals=tables)
    plain = host.query_nearest(sc, rows, channels=names)
    for k in names:
        assert walk[k].tobytes() == plain[k].tobytes(), f"{k}: the channels are query_nearest's, bit for bit"
    assert same(np.abs(walk["signed_distance"]), walk["distance"]), "distance == |signed| bit for bit"
    assert set(np.unique(walk["feature"])) >= {1, 2, 3, 4, 5}
    full = host.query_signed_distance(sc, rows, channels=names, pseudonormals=tables, exhaustive=True)
    one = (walk["object_id"] == full["object_id"]) & (walk["triangle_id"] == full["triangle_id"])
    assert one.mean() > 0.9
    assert same(walk["signed_distance"][one], full["signed_distance"][one]) and (walk["feature"][one] == full["feature"][one]).all()
    # masks: mask 0 rows are unanswered; hidden objects own no row; the filtered channels are the filtered query's
    om = np.array([1, 2, 4, 8, 16], np.uint32)
    rm = np.where(np.arange(600) % 3 == 0, 0, rng.integers(1, 32, 600)).astype(np.uint32)
    f = host.query_signed_distance(sc, rows, channels=names, pseudonormals=tables, mask=rm, object_masks=om)
    g = host.query_nearest(sc, rows, channels=names, mask=rm, object_masks=om)
    for k in names:
        assert f[k].tobytes() == g[k].tobytes(), k
    dead = rm == 0
    assert np.isposinf(f["signed_distance"][dead]).all() and (f["feature"][dead] == 0).all()
    seen = f["object_id"] >= 0
    assert ((om[f["object_id"][seen]] & rm[seen]) != 0).all()
    fe = host.query_signed_distance(sc, rows, channels=names, pseudonormals=tables, mask=rm, object_masks=om, exhaustive=True)
    one = (f["object_id"] == fe["object_id"]) & (f["triangle_id"] == fe["triangle_id"])
    assert same(f["signed_distance"][one], fe["signed_distance"][one])
    # a mesh without tables beside one with: + 8 for its rows only
    half = host.query_signed_distance(sc, rows, channels=("object_id",), pseudonormals={0: tables[0]})
    tri = half["object_id"] < 2
    assert ((half["feature"][tri] >= 8) == (half["object_id"][tri] == 1)).all() and (half["feature"][~tri & (half["object_id"] >= 0)] < 8).all()


def test_host_twin_refuses_bad_arguments(host):
    sc, meshes = rules_scene()
    rows = ss.as_rows(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        host.query_signed_distance(sc, rows, pseudonormals={7: ss.host_tables(meshes)[0]})
    with pytest.raises(ValueError):
        host.query_signed_distance(sc, rows, pseudonormals={0: ss.host_tables(meshes)[0][:2]})
    s, keep = host.nearest_scene(sc)
    out = np.zeros(2, f32)
    lib = host.lib()
    assert lib.rtxh_query_signed_distance(C.byref(s), rows.ctypes.data, 2, 0, None, None, None, None, None) == 1, "signed_out is required"
    assert lib.rtxh_query_signed_distance(C.byref(s), rows.ctypes.data, 2, 1, None, None, out.ctypes.data, None, None) == 1, "channels without out"
    assert lib.rtxh_query_signed_distance(C.byref(s), rows.ctypes.data, 2, 0, None, None, out.ctypes.data, None, None) == 0
    assert lib.rtxh_blas_pseudonormals(None, None, 1, 1, None, 0, None, None) == 1


def test_python_checks_come_before_the_library():
    torch = pytest.importorskip("torch")
    from pyrtx import api
    r = _offline_renderer(api)
    pts = torch.zeros((4, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        r.query_signed_distance(torch.zeros((4, 3), dtype=torch.float32))
    with pytest.raises(TypeError):
        r.query_signed_distance(pts.double())
    with pytest.raises(ValueError):
        r.query_signed_distance(pts, channels=("depth",))
    with pytest.raises(ValueError):
        r.query_signed_distance(pts, out={"signed_distance": torch.zeros(3, dtype=torch.float32)})
    with pytest.raises(TypeError):
        r.query_signed_distance(pts, feature=True, out={"feature": torch.zeros(4, dtype=torch.float32)})
    with pytest.raises(ValueError):
        r.query_signed_distance(pts, out={"distance": torch.zeros(4, dtype=torch.float32)})
    with pytest.raises(ValueError):
        r.query_signed_distance(1234, n=4, out={})
    with pytest.raises(TypeError):
        r.blas_pseudonormals(0, torch.zeros((4, 3), dtype=torch.float64))
