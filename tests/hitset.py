"""Scenes and labelled segment classes for all-hits queries (Renderer.query_hits / host.query_hits), like pointset.py for points.  Plain
numpy and the host library; no oracle.

Scenes
  quad_stack_scene()      12 parallel quads (24 triangles) under a rotated pose, one sphere, one plane: a ray along the stack has 27 hits
  rotated_mesh_scene(s)   two generated closed bumpy spheres, one inside the other, and a generated open sheet, all rotated at random into the
                          vertices (identity instances: co == o exactly), no axis-aligned face: the benign sets
  slab_chain_scene()      a chain BVH over 24 slabs across x: chain_rays() cross all of them with 23 stack entries (past RTX_LDS_STACK)
  cube_pose_scene()       the closed `cube` mesh under a rotated, translated pose; inside_cube() is its analytic inside test

Segment classes of generate(sc, n, seed) (n of each, fewer where the scene has no such geometry), max distance +inf unless noted
  incoherent   origins uniform in the inflated world box, directions uniform on the sphere
  through      aimed at a point inside a random triangle from outside the world box: crosses everything on the way
  grazing      nearly in the plane of a triangle (1e-3 .. 1e-6 off it), through its centroid
  edges        aimed at triangle vertices and edge midpoints (shared edges, shared vertices), half of them along a coordinate axis
  surface      starting on the fp32 hit point of an earlier segment, in a fresh direction (t near RAY_EPSILON and near 0)
  axial        a direction along one axis: two components +-0 (infinite inverses), origin in the world box
  box_planes   origins exactly on a plane of a TLAS or (identity-rotation instances) BLAS node box, the direction +-0 on that axis
  on_hit       an earlier segment again with its max distance exactly on one of its hits, one ulp below and one ulp above it
  short        max distances of 0.01 .. 2 scene sizes
  dead         zero direction, NaN / infinite components, max distance NaN, 0, -0, negative, -inf"""
import copy

import numpy as np

import util

f32 = np.float32
CLASSES = ("incoherent", "through", "grazing", "edges", "surface", "axial", "box_planes", "on_hit", "short", "dead")
ALL = ("distance", "position", "normal", "uv", "material_id", "object_id", "triangle_id")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _xform(m16, p):
    m = np.asarray(m16, np.float64).reshape(4, 4)
    return np.asarray(p, np.float64) @ m[:3, :3].T + m[:3, 3]


def mesh_scene(meshes, poses=None, spheres=(), planes=()):
    """cube's materials, lights and config around generated meshes: meshes = [(n, 3, 3) float triangle soups], poses = [(position,
    unit quaternion xyzw)] per mesh (identity when None), spheres = [(centre, radius)], planes = [(normal, distance)] with unit normals."""
    from pyrtx import host, scene_io as sio
    sc = copy.deepcopy(util.load_golden("cube")[0])
    mat = int(sc.blas[0].tri_cold["material_id"][0]); off = sc.blas[0].material_offset
    sc.blas, insts, boxes, centres = [], [], [], []
    for k, tris in enumerate(meshes):
        tris = np.asarray(tris, f32).reshape(-1, 3, 3)
        n = len(tris)
        e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
        nrm = np.cross(e1, e2).astype(np.float64); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
        normals = np.repeat(nrm[:, None, :], 3, axis=1).astype(f32)
        uv = np.tile(np.array([[0, 0], [1, 0], [0, 1]], f32), (n, 1, 1))
        sc.blas.append(host.build_blas(tris, normals, uv, np.full(n, mat, np.int32), off, reference_bvh=True))
        root = sc.blas[-1].nodes[0]
        pos, rot = poses[k] if poses else ((0, 0, 0), (0, 0, 0, 1))
        inst, mn, mx = host.instance_update(pos, rot, root["aabb_min"], root["aabb_max"], k)
        insts.append(inst); boxes.append(np.concatenate([mn, mx])); centres.append(0.5 * (mn + mx))
    sc.instances = np.concatenate(insts)
    sc.tlas_nodes, sc.tlas_indices = host.Tlas(len(meshes)).build(np.array(centres, f32), np.array(boxes, f32))
    sc.spheres = np.zeros(len(spheres), sio.SPHERE)
    for i, (c, r) in enumerate(spheres):
        sc.spheres[i]["center"] = c; sc.spheres[i]["radius_squared"] = f32(r) * f32(r); sc.spheres[i]["radius_inv"] = f32(1) / f32(r); sc.spheres[i]["material_id"] = 0
    sc.planes = np.zeros(len(planes), sio.PLANE)
    for i, (nv, d) in enumerate(planes):
        nv = np.asarray(nv, np.float64)
        u = np.cross(nv, [0.0, 0.0, 1.0] if abs(nv[2]) < 0.9 else [1.0, 0.0, 0.0]); u /= np.linalg.norm(u)
        sc.planes[i]["normal"] = nv; sc.planes[i]["distance"] = d; sc.planes[i]["u_axis"] = u; sc.planes[i]["v_axis"] = np.cross(nv, u); sc.planes[i]["material_id"] = 0
    return sc


QUAD_POSE = ((0.5, -0.25, 6.0), (0.18257419, 0.36514837, 0.54772256, 0.73029674))      # (1, 2, 3, 4) / sqrt(30)


def quad_stack_scene():
    """12 quads of side 4 at z = -2.75, -2.25, .. 2.75 in the mesh's space, each turned a little further about z, under QUAD_POSE; a sphere
    of radius 1.5 around the stack's middle and a plane behind it."""
    tris = []
    for k in range(12):
        a = 0.2 * k
        c, s = np.cos(a), np.sin(a)
        corners = np.array([[-2, -2], [2, -2], [2, 2], [-2, 2]], np.float64) @ np.array([[c, s], [-s, c]])
        q = np.concatenate([corners, np.full((4, 1), -2.75 + 0.5 * k)], axis=1)
        tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return mesh_scene([np.array(tris)], [QUAD_POSE], spheres=[(QUAD_POSE[0], 1.5)], planes=[((0.0, 0.6, 0.8), -12.0)])


def slab_chain_scene(n=24):
    """One mesh whose BVH is a chain (every inner node = one leaf + the rest, inner depth n - 2) over n slabs across the x axis: a segment
    along -x from beyond the last slab enters the rest first at every step and leaves the leaf on the stack — n - 1 entries, n hits."""
    from pyrtx import scene_io as sio
    sc = mesh_scene([np.zeros((1, 3, 3))])
    hot = np.zeros(n, sio.TRI_HOT); cold = np.zeros(n, sio.TRI_COLD)
    for i in range(n):
        hot["position_0"][i] = (i * 0.25 - 3.0, -1.0 - 0.01 * (i % 3), -1.0); hot["position_edge_1"][i] = (0.02, 2.5, 0.1 * (i % 2)); hot["position_edge_2"][i] = (-0.02, 0.1, 2.5)
        cold["normal_0"][i] = (-1, 0, 0); cold["material_id"][i] = sc.blas[0].tri_cold["material_id"][0]
        cold["tex_coord_edge_1"][i] = (1, 0); cold["tex_coord_edge_2"][i] = (0, 1)
    box = lambda t: np.stack([hot["position_0"][t], hot["position_0"][t] + hot["position_edge_1"][t], hot["position_0"][t] + hot["position_edge_2"][t]])
    nodes = np.zeros(2 * n - 1, sio.BVH_NODE)
    for d in range(n - 1):                                            # the inner node of chain step d is node 2d; its children (leaf d, the rest) are 2d + 1, 2d + 2
        k = 2 * d
        nodes[k]["left_or_first"] = 2 * d + 1; nodes[k]["count"] = np.uint32((1 + d % 3) << 30).astype(np.int32)
        nodes[2 * d + 1]["left_or_first"] = d; nodes[2 * d + 1]["count"] = 1
        b = box(d); nodes[2 * d + 1]["aabb_min"] = b.min(axis=0); nodes[2 * d + 1]["aabb_max"] = b.max(axis=0)
    last = 2 * (n - 1)
    nodes[last]["left_or_first"] = n - 1; nodes[last]["count"] = 1
    b = box(n - 1); nodes[last]["aabb_min"] = b.min(axis=0); nodes[last]["aabb_max"] = b.max(axis=0)
    for d in range(n - 2, -1, -1):                                    # inner boxes bottom-up
        k, l = 2 * d, 2 * d + 1
        nodes[k]["aabb_min"] = np.minimum(nodes[l]["aabb_min"], nodes[l + 1]["aabb_min"]); nodes[k]["aabb_max"] = np.maximum(nodes[l]["aabb_max"], nodes[l + 1]["aabb_max"])
    sc.blas[0] = sio.Blas(nodes, hot, cold, sc.blas[0].material_offset, n)
    sc.tlas_nodes = sc.tlas_nodes.copy()                              # the one instance is unrotated at the origin: its leaf gets the new root box
    sc.tlas_nodes[0]["aabb_min"] = nodes[0]["aabb_min"]; sc.tlas_nodes[0]["aabb_max"] = nodes[0]["aabb_max"]
    return sc


def chain_rays(n=6):
    """Segments along -x through all of slab_chain_scene()'s slabs."""
    seg = np.zeros((n, 7), f32)
    seg[:, 0] = 4.0; seg[:, 1] = np.linspace(-0.4, 0.3, n); seg[:, 2] = np.linspace(0.2, -0.3, n); seg[:, 3] = -1.0; seg[:, 4] = 0.01; seg[:, 6] = np.inf
    return seg


def bumpy_sphere(rng, rings=7, sectors=10, radius=2.0):
    """A closed, bumpy lat-long sphere as a triangle soup, (n, 3, 3) float64."""
    r = radius * (1 + 0.25 * rng.uniform(-1, 1, (rings + 1, sectors)))
    r[0, :] = r[0, 0]; r[rings, :] = r[rings, 0]
    th = np.pi * np.arange(rings + 1) / rings
    ph = 2 * np.pi * (np.arange(sectors) + 0.37) / sectors
    p = np.stack([r * np.sin(th)[:, None] * np.cos(ph)[None, :], r * np.sin(th)[:, None] * np.sin(ph)[None, :], r * np.cos(th)[:, None] * np.ones(sectors)[None, :]], axis=-1)
    tris = []
    for i in range(rings):
        for j in range(sectors):
            a, b, c, d = p[i, j], p[i, (j + 1) % sectors], p[i + 1, (j + 1) % sectors], p[i + 1, j]
            if i > 0: tris.append([a, b, c])
            if i < rings - 1: tris.append([a, c, d])
    return np.array(tris)


def sheet(rng, nu=6, nv=6, size=5.0):
    """An open wavy sheet, (n, 3, 3) float64."""
    u, v = np.meshgrid(np.linspace(-size / 2, size / 2, nu + 1), np.linspace(-size / 2, size / 2, nv + 1), indexing="ij")
    p = np.stack([u, v, 0.4 * rng.uniform(-1, 1, u.shape)], axis=-1)
    tris = []
    for i in range(nu):
        for j in range(nv):
            tris += [[p[i, j], p[i + 1, j], p[i + 1, j + 1]], [p[i, j], p[i + 1, j + 1], p[i, j + 1]]]
    return np.array(tris)


def rotated_mesh_scene(seed):
    """The benign scene of a seed: two nested bumpy spheres and a sheet through them, each rotated at random (into the vertices) and
    shifted, identity instances: a segment through the middle has six or seven hits."""
    rng = np.random.default_rng(seed)
    a = bumpy_sphere(rng, radius=2.4) @ _rotation(rng).T + rng.uniform(-0.2, 0.2, 3)
    b = bumpy_sphere(rng, 6, 8, radius=1.2) @ _rotation(rng).T + rng.uniform(-0.2, 0.2, 3)
    c = sheet(rng) @ _rotation(rng).T + rng.uniform(-0.3, 0.3, 3)
    return mesh_scene([a, b, c])


CUBE_POSE = ((1.25, -0.5, 7.0), (0.36514837, -0.18257419, 0.73029674, 0.54772256))


def cube_pose_scene():
    """The closed `cube` mesh (its own BLAS) under CUBE_POSE: one instance, no spheres, no planes."""
    from pyrtx import host, scene_io as sio
    sc = copy.deepcopy(util.load_golden("cube")[0])
    sc.blas = [sc.blas[int(sc.instances[0]["blas_id"])]]
    root = sc.blas[0].nodes[0]
    inst, mn, mx = host.instance_update(CUBE_POSE[0], CUBE_POSE[1], root["aabb_min"], root["aabb_max"], 0)
    sc.instances = inst
    sc.tlas_nodes, sc.tlas_indices = host.Tlas(1).build((0.5 * (mn + mx))[None], np.concatenate([mn, mx])[None])
    sc.spheres = np.zeros(0, sio.SPHERE); sc.planes = np.zeros(0, sio.PLANE)
    return sc


def inside_cube(sc, points, margin=0.0):
    """(inside, clear): the analytic side of world points against cube_pose_scene()'s mesh — an axis-aligned box in its own space — in
    float64; clear = farther than `margin` from every face."""
    root = sc.blas[0].nodes[0]
    pl = _xform(sc.instances[0]["world_inv"], points)
    lo, hi = root["aabb_min"].astype(np.float64), root["aabb_max"].astype(np.float64)
    inside = ((pl > lo) & (pl < hi)).all(axis=1)
    clear = (np.minimum(np.abs(pl - lo), np.abs(pl - hi)) > margin).all(axis=1)
    return inside, clear


def world_box(sc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    if len(sc.tlas_nodes):
        lo = np.minimum(lo, sc.tlas_nodes[0]["aabb_min"]); hi = np.maximum(hi, sc.tlas_nodes[0]["aabb_max"])
    for s in sc.spheres:
        r = np.sqrt(float(s["radius_squared"]))
        lo = np.minimum(lo, s["center"] - r); hi = np.maximum(hi, s["center"] + r)
    if not np.all(np.isfinite(lo)):
        lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    ext = np.maximum(hi - lo, 1e-3)
    return lo - 0.25 * ext, hi + 0.25 * ext


def _triangle(sc, rng):
    insts = np.asarray(sc.tlas_indices)
    inst = sc.instances[int(insts[rng.integers(len(insts))])]
    hot = sc.blas[int(inst["blas_id"])].tri_hot
    t = hot[int(rng.integers(len(hot)))]
    return inst, t["position_0"].astype(np.float64), t["position_edge_1"].astype(np.float64), t["position_edge_2"].astype(np.float64)


def _identity_rotation(inst):
    return np.array_equal(np.asarray(inst["world_inv"], f32).reshape(4, 4)[:3, :3], np.eye(3, dtype=f32))


def generate(sc, n=20, seed=0):
    """-> (segments float32 (N, 7), labels int (N,) into CLASSES), N about 12 n."""
    from pyrtx import host
    rng = np.random.default_rng(seed)
    lo, hi = world_box(sc)
    size = float(np.max(hi - lo))
    mid = 0.5 * (lo + hi)
    parts = {}
    has_tris = len(sc.tlas_indices) > 0

    def rows(o, d, D=np.inf):
        o, d = np.atleast_2d(o), np.atleast_2d(d)
        return np.concatenate([o, d, np.broadcast_to(np.asarray(D, np.float64).reshape(-1, 1), (len(o), 1))], axis=1).astype(f32)

    parts["incoherent"] = rows(rng.uniform(lo, hi, (n, 3)), _unit(rng, n) * rng.uniform(0.3, 3.0, (n, 1)))
    thr, gra, edg = [], [], []
    for k in range(n if has_tris else 0):
        inst, p0, e1, e2 = _triangle(sc, rng)
        target = _xform(inst["world"], p0 + rng.uniform(0.1, 0.4) * e1 + rng.uniform(0.1, 0.4) * e2)
        o = mid + _unit(rng, 1)[0] * size * rng.uniform(0.8, 1.5)
        thr.append(rows(o, (target - o) * rng.uniform(0.2, 2.0)))
        nrm = np.cross(e1, e2); ln = np.linalg.norm(nrm)
        if ln > 0:                                                         # nearly in the triangle's plane, through its centroid
            nrm /= ln
            along = e1 / np.linalg.norm(e1) * np.cos(0.7 * k) + np.cross(nrm, e1 / np.linalg.norm(e1)) * np.sin(0.7 * k)
            d_l = along + nrm * (10.0 ** rng.uniform(-6, -3)) * (1 if k % 2 else -1)
            c_l = p0 + (e1 + e2) / 3
            m = np.asarray(inst["world"], np.float64).reshape(4, 4)[:3, :3]
            gra.append(rows(_xform(inst["world"], c_l - d_l * rng.uniform(0.5, 2.0) * size), m @ d_l))
        corner = [p0, p0 + e1, p0 + e2, p0 + e1 / 2, p0 + e2 / 2, p0 + (e1 + e2) / 2][int(rng.integers(6))]
        tg = _xform(inst["world"], corner).astype(f32).astype(np.float64)
        if k % 2:
            ax = int(rng.integers(3)); sgn = 1.0 if rng.random() < 0.5 else -1.0
            o = tg.copy(); o[ax] -= sgn * size
            d = np.zeros(3); d[ax] = sgn
        else:
            o = rng.uniform(lo, hi); d = tg - o
        edg.append(rows(o, d))
    if thr:
        parts["through"], parts["edges"] = np.concatenate(thr), np.concatenate(edg)
    if gra:
        parts["grazing"] = np.concatenate(gra)
    ax = rng.integers(3, size=n)
    d = np.zeros((n, 3)); d[np.arange(n), ax] = rng.choice([-1.0, 1.0, 0.5, -2.0], n)
    d[np.arange(n), (ax + 1) % 3] = rng.choice([0.0, -0.0], n)
    o = rng.uniform(lo, hi, (n, 3)); o[np.arange(n), ax] = np.where(d[np.arange(n), ax] > 0, lo[ax], hi[ax])
    parts["axial"] = rows(o, d)
    bp = []
    for k in range(n if has_tris else 0):
        use_blas = [i for i in np.asarray(sc.tlas_indices) if _identity_rotation(sc.instances[int(i)])]
        if k % 2 and use_blas:                                             # a BLAS node plane through an unrotated instance: local = world + c, inverted when exact
            inst = sc.instances[int(use_blas[int(rng.integers(len(use_blas)))])]
            nodes = sc.blas[int(inst["blas_id"])].nodes
            c = np.asarray(inst["world_inv"], f32).reshape(4, 4)[:3, 3]
        else:
            nodes, c = sc.tlas_nodes, np.zeros(3, f32)
        node = nodes[int(rng.integers(len(nodes)))]
        if not (np.isfinite(node["aabb_min"]).all() and np.isfinite(node["aabb_max"]).all()):
            continue
        a = int(rng.integers(3))
        plane = f32(node["aabb_min"][a] if rng.random() < 0.5 else node["aabb_max"][a])
        x = f32(plane - c[a])
        if f32(x + c[a]) != plane:
            continue
        o = (rng.uniform(node["aabb_min"] - 0.3, node["aabb_max"] + 0.3) - c).astype(f32)
        o[a] = x
        d = _unit(rng, 1)[0]
        d[a] = -0.0 if rng.random() < 0.5 else 0.0
        bp.append(rows(o, d))
    if bp:
        parts["box_planes"] = np.concatenate(bp)
    so_far = np.concatenate(list(parts.values()))
    h = host.query_hits(sc, so_far, 8, ("distance", "position"))
    hit = np.flatnonzero(h["count"] > 0)
    if len(hit):
        pick = hit[rng.integers(len(hit), size=n)]
        j = np.array([rng.integers(min(int(h["count"][i]), 8)) for i in pick])
        parts["surface"] = rows(h["position"][pick, j], _unit(rng, n))
        t = h["distance"][pick, j]
        on = [np.concatenate([so_far[pick, :6], D[:, None]], axis=1) for D in (t, np.nextafter(t, f32(-np.inf)), np.nextafter(t, f32(np.inf)))]
        parts["on_hit"] = np.concatenate(on).astype(f32)
    parts["short"] = rows(rng.uniform(lo, hi, (n, 3)), _unit(rng, n), size * 10.0 ** rng.uniform(-2, 0.3, n))
    m = mid.astype(f32)
    dead = [[*m, 0, 0, 0, np.inf], [*m, -0.0, 0.0, -0.0, 5], [np.nan, m[1], m[2], 1, 0, 0, np.inf], [m[0], np.inf, m[2], 0, 1, 0, np.inf], [*m, np.nan, 0, 1, np.inf],
            [*m, 0, -np.inf, 1, np.inf], [*m, 1, 0, 0, np.nan], [*m, 1, 0, 0, 0.0], [*m, 1, 0, 0, -0.0], [*m, 0, 1, 0, -3.0], [*m, 0, 0, 1, -np.inf]]
    parts["dead"] = np.array(dead, f32)
    seg = np.concatenate([parts[k] for k in CLASSES if k in parts]).astype(f32)
    lab = np.concatenate([np.full(len(parts[k]), CLASSES.index(k)) for k in CLASSES if k in parts])
    return np.ascontiguousarray(seg), lab


def is_dead(seg):
    """The dead-row rule of include/rtx.h, restated."""
    seg = np.asarray(seg, f32)
    with np.errstate(invalid="ignore"):
        return (seg[:, 3:6] == 0).all(axis=1) | ~np.isfinite(seg[:, :6]).all(axis=1) | ~(seg[:, 6] > 0)
