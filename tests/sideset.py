"""Shared inputs of the signed-distance tests (tests/test_query_signed_cpu.py, tests/test_gpu_query_signed.py): scenes of posed golden meshes
with their slot -> vertex tables, a numpy float64 restatement of the pseudonormal tables (csrc/rtx_side_math.h) written per triangle and per
undirected edge, the float64 generalized winding number of posed triangles (the independent oracle of the sign), a float64 nearest-feature
search for the rows the specification leaves undetermined, and the open sheets."""
import copy
import functools

import numpy as np

import normalset as ns
import util

f32, f64 = np.float32, np.float64
CLOSED = ("Cube", "Diamond", "Rock", "Torus", "icosphere")
# Largest angle between a record of the twin and the float64 restatement on Cube, Diamond, Rock, Torus, icosphere and Monkey (vertex and edge
# records whose float64 length is above 1e-3), as measured: 9.19e-7 radians (a vertex of Monkey; the closed meshes stay below 1.4e-7).  DELTA = four times it: the margin covers other valences
# and the ulp spread of rtx_atan2f (Signed distance).
MEASURED_DEVIATION = 9.19e-7
DELTA = 4 * MEASURED_DEVIATION


# ---- float64 restatement of the tables -----------------------------------------------------------------------------------------------------
def tables64(pos, idx, sv):
    """-> (vert (V, 3), edge (slots, 3, 3), unit face normals (T, 3)) in float64, from the float32 inputs."""
    p = np.asarray(pos, f64); idx = np.asarray(idx, np.int64).reshape(-1, 3); sv = np.asarray(sv, np.int64).reshape(-1, 3)
    V = len(p)
    ok = ns.valid_triangles(idx, V)
    tri = p[np.where(ok[:, None], idx, 0)]
    f = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    L = np.linalg.norm(f, axis=1)
    good = ok & (L > 0)
    n = np.where(good[:, None], f / np.where(L > 0, L, 1)[:, None], 0.0)
    vert = np.zeros((V, 3), f64)
    pairs = {}
    for t in np.nonzero(good)[0]:
        for k in range(3):
            ea, eb = tri[t, (k + 1) % 3] - tri[t, k], tri[t, (k + 2) % 3] - tri[t, k]
            vert[idx[t, k]] += np.arctan2(L[t], ea @ eb) * n[t]
        i = idx[t]
        for a, b in ((i[0], i[1]), (i[1], i[2]), (i[0], i[2])):
            key = (min(a, b), max(a, b))
            pairs[key] = pairs.get(key, 0) + n[t]
    edge = np.zeros((len(sv), 3, 3), f64)
    for s, (a, b, c) in enumerate(sv):
        for k, (x, y) in enumerate(((a, b), (b, c), (a, c))):
            if 0 <= x < V and 0 <= y < V:
                edge[s, k] = pairs.get((min(x, y), max(x, y)), 0)
    return vert, edge, n


def angle_between(a, b):
    a = np.asarray(a, f64); b = np.asarray(b, f64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))


# ---- meshes as BLAS -------------------------------------------------------------------------------------------------------------------------
def mesh_blas(pos, idx, **kw):
    """An indexed mesh as (scene_io.Blas built by host.build_blas, slot -> vertex table (slots, 3) int32); flat face normals in the cold records."""
    from pyrtx import host
    pos = np.ascontiguousarray(pos, f32); idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    soup = pos[idx]
    with np.errstate(all="ignore"):
        fn = np.cross(soup[:, 1] - soup[:, 0], soup[:, 2] - soup[:, 0]).astype(f64)
        fn = fn / np.maximum(np.linalg.norm(fn, axis=1), 1e-30)[:, None]
    nrm = np.repeat(fn[:, None, :], 3, 1).astype(f32)
    blas = host.build_blas(soup, nrm, np.zeros((len(idx), 3, 2), f32), np.zeros(len(idx), np.int32), 0, **kw)
    return blas, host.slot_vertices(blas, idx)


@functools.lru_cache(maxsize=None)
def golden_mesh(name, sbvh=False):
    pos, idx = ns.indexed(name)
    blas, sv = mesh_blas(pos, idx, **({"reference_sbvh": True} if sbvh else {}))
    return pos, idx, blas, sv


def random_quaternions(n, rng):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1)[:, None]).astype(f32)


def world_box(inst, pos):
    """float64 box of the vertices `pos` through the instance's float32 world matrix, padded by 1e-5 of its size."""
    w = np.asarray(inst["world"], f64).reshape(4, 4)
    q = np.asarray(pos, f64) @ w[:3, :3].T + w[:3, 3]
    mn, mx = q.min(0), q.max(0)
    pad = 1e-5 * float((mx - mn).max()) + 1e-6
    return mn - pad, mx + pad


def posed_scene(meshes, positions, rotations, mirrored=(), spheres=None, planes=None):
    """cube's config, materials and lights; one instance per entry of meshes = [(pos, idx, blas, sv)], BLAS id = its index, posed by the
    unit quaternions and translations through the project's own Mesh::update; instances listed in `mirrored` are reflected in their local x
    (world = world . diag(-1, 1, 1), world_inv = diag(-1, 1, 1) . world_inv: sign flips, exact).  The TLAS is the balanced one over float64
    boxes of the posed vertices."""
    from pyrtx import host, scene_io as sio
    sc = copy.deepcopy(util.load_golden("cube")[0])
    sc.blas = [m[2] for m in meshes]
    n = len(meshes)
    inst = np.zeros(n, sio.INSTANCE)
    aabbs = np.zeros((n, 6), f32)
    for i, m in enumerate(meshes):
        root = m[2].nodes[0]
        one, _, _ = host.instance_update(positions[i], rotations[i], root["aabb_min"], root["aabb_max"], i)
        inst[i] = one[0]
        if i in mirrored:
            w = inst["world"][i].reshape(4, 4).copy(); wi = inst["world_inv"][i].reshape(4, 4).copy()
            w[:, 0] = -w[:, 0]; wi[0, :] = -wi[0, :]
            inst["world"][i] = w.reshape(16); inst["world_inv"][i] = wi.reshape(16)
        mn, mx = world_box(inst[i], m[0])
        aabbs[i, :3] = np.nextafter(mn.astype(f32), f32(-np.inf)); aabbs[i, 3:] = np.nextafter(mx.astype(f32), f32(np.inf))
    sc.instances = inst
    sc.tlas_nodes, sc.tlas_indices = host.tlas_build_balanced(np.asarray(positions, f32), aabbs)
    sc.spheres = np.zeros(0, sio.SPHERE) if spheres is None else spheres
    sc.planes = np.zeros(0, sio.PLANE) if planes is None else planes
    return sc


def posed_triangles(sc, meshes):
    """float64 world-space triangles (sum T, 3, 3) of every instance, in instance order, and the instance of each."""
    tris, owner = [], []
    for i, m in enumerate(meshes):
        w = np.asarray(sc.instances["world"][i], f64).reshape(4, 4)
        q = np.asarray(m[0], f64) @ w[:3, :3].T + w[:3, 3]
        tris.append(q[np.asarray(m[1], np.int64)]); owner.append(np.full(len(m[1]), i))
    return np.concatenate(tris), np.concatenate(owner)


def host_tables(meshes):
    """{blas_id: (vert, edge, slot_vertices)} through the twin, for host.query_signed_distance."""
    from pyrtx import host
    return {i: host.blas_pseudonormals(m[0], m[1], m[3]) + (m[3],) for i, m in enumerate(meshes)}


# ---- the oracle: generalized winding number (van Oosterom and Strackee's solid angle, summed) ---------------------------------------------
def winding_number(points, tris, chunk=256):
    P = np.asarray(points, f64); out = np.zeros(len(P), f64)
    for s in range(0, len(P), chunk):
        a = tris[None, :, 0] - P[s:s + chunk, None]; b = tris[None, :, 1] - P[s:s + chunk, None]; c = tris[None, :, 2] - P[s:s + chunk, None]
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = (a * np.cross(b, c)).sum(2)
        den = la * lb * lc + (a * b).sum(2) * lc + (b * c).sum(2) * la + (c * a).sum(2) * lb
        out[s:s + chunk] = (2 * np.arctan2(num, den)).sum(1) / (4 * np.pi)
    return out


# ---- float64 nearest feature: what the specification's leave-out rule is stated in --------------------------------------------------------
def nearest64(P, A, E1, E2, chunk=256):
    """For every point the nearest of the triangles (A, E1, E2) in float64 by the Voronoi regions of Ericson 5.1.5 -> (triangle, region code
    of rtx_side_math.h, r = p - closest point, squared distance)."""
    P = np.asarray(P, f64)
    best_t = np.zeros(len(P), np.int64); best_reg = np.zeros(len(P), np.int64); best_r = np.zeros((len(P), 3)); best_d2 = np.full(len(P), np.inf)
    aa, ab, cc = (E1 * E1).sum(1), (E1 * E2).sum(1), (E2 * E2).sum(1)
    for s in range(0, len(P), chunk):
        ap = P[s:s + chunk, None] - A[None]
        d1, d2 = (ap * E1[None]).sum(2), (ap * E2[None]).sum(2)
        d3, d4, d5, d6 = d1 - aa, d2 - ab, d1 - ab, d2 - cc
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(all="ignore"):
            conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                     (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); k = 1 / (va + vb + vc)
            u = np.select(conds, [0 * d1, 1 + 0 * d1, d1 / (d1 - d3), 0 * d1, 0 * d1, 1 - w], vb * k)
            v = np.select(conds, [0 * d1, 0 * d1, 0 * d1, 1 + 0 * d1, d2 / (d2 - d6), w], vc * k)
        reg = np.select(conds, [0, 1, 3, 2, 5, 4], 6)
        r = ap - (u[..., None] * E1[None] + v[..., None] * E2[None])
        dd = (r * r).sum(2)
        dd = np.where(np.isfinite(dd), dd, np.inf)
        t = dd.argmin(1); rows = np.arange(len(t))
        best_t[s:s + chunk] = t; best_reg[s:s + chunk] = reg[rows, t]; best_r[s:s + chunk] = r[rows, t]; best_d2[s:s + chunk] = dd[rows, t]
    return best_t, best_reg, best_r, best_d2


def undetermined(sc, meshes, points):
    """The rows the specification leaves out, from float64 alone: the nearest instance's nearest feature in that instance's local space ->
    (left_out (n,) bool, float64 distance (n,)).  A row is left out when its distance is at most rtxh_nearest_distance_bound(S, W), or
    |cos(r, N)| is at most bound / |r| + DELTA, N the float64 pseudonormal of the feature."""
    from pyrtx import host
    P = np.asarray(points, f64)[:, :3]
    n = len(P)
    best = np.full(n, np.inf); out = np.zeros(n, bool)
    for i, m in enumerate(meshes):
        wi = np.asarray(sc.instances["world_inv"][i], f64).reshape(4, 4)
        pl = P @ wi[:3, :3].T + wi[:3, 3]
        pos, idx, _, _ = m
        vert, edge, _ = tables64(pos, idx, idx)
        tri = np.asarray(pos, f64)[np.asarray(idx, np.int64)]
        A, E1, E2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        t, reg, r, d2 = nearest64(pl, A, E1, E2)
        d = np.sqrt(d2)
        N = np.where((reg == 6)[:, None], np.cross(E1[t], E2[t]), 0.0)
        for k in range(3):
            N = np.where((reg == k)[:, None], vert[np.asarray(idx, np.int64)[t, k]], N)
            N = np.where((reg == 3 + k)[:, None], edge[t, k], N)
        S = np.linalg.norm(pl - A[t], axis=1) + np.linalg.norm(E1[t], axis=1) + np.linalg.norm(E2[t], axis=1)
        W = np.linalg.norm(P, axis=1) + np.linalg.norm(pl, axis=1)
        bound = np.array([host.nearest_distance_bound(float(s), float(w)) for s, w in zip(S, W)])
        with np.errstate(all="ignore"):
            cos = np.abs((r * N).sum(1)) / (d * np.linalg.norm(N, axis=1))
            leave = (d <= bound) | ~(cos > bound / d + DELTA)
        nearer = d < best
        out = np.where(nearer, leave, out); best = np.where(nearer, d, best)
    return out, best


# ---- the rows of the sign tests --------------------------------------------------------------------------------------------------------------
def closed_scene(seed=11):
    """The five closed golden meshes side by side, each posed by a random unit quaternion and translation, plus a mirrored Rock."""
    rng = np.random.default_rng(seed)
    meshes = [golden_mesh(name) for name in CLOSED] + [golden_mesh("Rock")]
    rot = random_quaternions(len(meshes), rng)
    radius = [float(np.linalg.norm(np.asarray(m[0], f64), axis=1).max()) for m in meshes]
    pos = np.zeros((len(meshes), 3), f32)
    x = 0.0
    for i, r in enumerate(radius):
        x += r
        pos[i] = (x, rng.uniform(-0.3, 0.3) * r, rng.uniform(-0.3, 0.3) * r + (i % 2) * 0.5 * r)
        x += r * 1.02
    return posed_scene(meshes, pos, rot, mirrored=(len(meshes) - 1,)), meshes


def uniform_rows(sc, meshes, count, rng):
    tris, _ = posed_triangles(sc, meshes)
    mn, mx = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, h = (mn + mx) / 2, (mx - mn) / 2 * 1.25
    return rng.uniform(c - h, c + h, (count, 3))


def feature_rows(sc, meshes, which):
    """Points offset to both sides of every edge midpoint and every vertex of the instances in `which`, by 1e-3 of the mesh size along the
    float64 pseudonormal, in world space."""
    rows = []
    for i in which:
        pos, idx, _, _ = meshes[i]
        p = np.asarray(pos, f64); ii = np.asarray(idx, np.int64)
        vert, edge, _ = tables64(pos, idx, idx)
        size = float((p.max(0) - p.min(0)).max())
        unit = lambda a: a / np.maximum(np.linalg.norm(a, axis=1), 1e-30)[:, None]
        used = np.unique(ii)
        base = [p[used]]; nrm = [unit(vert[used])]
        for k, (a, b) in enumerate(((0, 1), (1, 2), (0, 2))):
            keep = ii[:, a] < ii[:, b]                                # each undirected edge of a closed mesh once
            base.append(((p[ii[:, a]] + p[ii[:, b]]) / 2)[keep]); nrm.append(unit(edge[:, k])[keep])
        base, nrm = np.concatenate(base), np.concatenate(nrm)
        local = np.concatenate([base + 1e-3 * size * nrm, base - 1e-3 * size * nrm])
        w = np.asarray(sc.instances["world"][i], f64).reshape(4, 4)
        rows.append(local @ w[:3, :3].T + w[:3, 3])
    return np.concatenate(rows)


def surface_rows(sc, meshes, per, rng):
    """`per` points of every instance exactly on its surface in float64 local space — vertices, edge midpoints, points inside faces, a
    third each — through the instance's world matrix.  Rounded to float32 and posed they are on the surface only to rounding: rows the
    specification leaves undetermined (within the distance bound), unless they come back + 0."""
    rows = []
    for i, (pos, idx, _, _) in enumerate(meshes):
        p = np.asarray(pos, f64); tri = p[np.asarray(idx, np.int64)]
        t = rng.integers(0, len(tri), per)
        w3 = rng.dirichlet((1, 1, 1), per)
        kind = np.arange(per) % 3
        w3[kind == 0] = (1, 0, 0); w3[kind == 1] = (0.5, 0.5, 0)
        local = (w3[:, :, None] * tri[t]).sum(1)
        w = np.asarray(sc.instances["world"][i], f64).reshape(4, 4)
        rows.append(local @ w[:3, :3].T + w[:3, 3])
    return np.concatenate(rows)


def as_rows(points, rmax=np.inf):
    out = np.full((len(points), 4), rmax, f32)
    out[:, :3] = np.asarray(points, f32)
    return out


def rules_scene():
    """A frame that mixes two meshes (icosphere, Diamond: posed by random unit quaternions), two spheres and a plane (y = -3)."""
    from pyrtx import scene_io as sio
    meshes = [golden_mesh("icosphere"), golden_mesh("Diamond")]
    spheres = np.zeros(2, sio.SPHERE)
    spheres["center"] = [[4, 0, 0], [-4, 1, 0.5]]; spheres["radius_squared"] = [f32(0.49), f32(2.25)]; spheres["radius_inv"] = 1 / np.sqrt(spheres["radius_squared"])
    planes = np.zeros(1, sio.PLANE)
    planes["normal"] = [[0, 1, 0]]; planes["distance"] = 3.0; planes["u_axis"] = [[1, 0, 0]]; planes["v_axis"] = [[0, 0, 1]]
    rot = random_quaternions(2, np.random.default_rng(8))
    sc = posed_scene(meshes, np.array([[0, 0, 0], [0.5, 2.5, 0]], f32), rot, spheres=spheres, planes=planes)
    return sc, meshes


# ---- open sheets ------------------------------------------------------------------------------------------------------------------------------
def sheet(n=4, fold=0.0):
    """An n x n grid of cells in the plane y = 0 (two triangles per cell, normals +y), x and z in [0, n]; fold: the rows beyond the middle row
    z = n / 2 are bent about it by that angle (positive: upwards, the upper side becomes concave)."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, z = j.astype(f64), i.astype(f64)
    y = np.zeros_like(x)
    far = z > n / 2
    dz = z - n / 2
    z = np.where(far, n / 2 + dz * np.cos(fold), z); y = np.where(far, dz * np.sin(fold), y)
    pos = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
    v = lambda a, b: a * (n + 1) + b
    idx = []
    for a in range(n):
        for b in range(n):
            idx += [[v(a, b), v(a + 1, b), v(a, b + 1)], [v(a, b + 1), v(a + 1, b), v(a + 1, b + 1)]]
    return pos, np.array(idx, np.int32)
