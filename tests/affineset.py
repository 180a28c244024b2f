"""Shared inputs of the non-rigid-matrix tests (tests/test_affine_cpu.py, tests/test_gpu_affine.py): golden scenes whose instance matrices are
scaled, mirrored, sheared or flattened — what a caller of the C ABI can hand to rtx_set_frame and no scene builder of this project makes —
a plain float64 world-space ray / triangle reference, and the numpy float32 restatement of csrc/rtx_math.h's xform_pos / xform_dir by which
every row is checked before a GPU test sends it.

with_linear(sc, Ls): instance i gets L = Ls[i % len(Ls)]: world <- world . L, world_inv <- L+ . world_inv (L+ the pseudo-inverse: the inverse
where there is one), formed in float64 from the float32 cells and rounded once; its world box is the box of the eight float64 corners of the
BLAS root box through the new world matrix, padded as sideset.world_box pads; the TLAS is host.tlas_build_balanced over those boxes."""
import copy
import functools

import numpy as np

import util

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                                       # one unit roundoff of float32
WIDTH, HEIGHT = 64, 48
BASES = ("cube", "materials")
I3 = np.eye(3)
LINEAR = {
    "uniform2": np.diag([2.0, 2.0, 2.0]),
    "uniform_half": np.diag([0.5, 0.5, 0.5]),
    "tiny": np.diag([2.0 ** -10] * 3),
    "nonuniform": np.diag([2.0, 0.5, 1.25]),
    "mirror": np.diag([-1.0, 1.0, 1.0]),
    "shear": np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 1.0]]),
    "flat": np.diag([1.0, 0.0, 1.0]),
}
MIXED = ("uniform2", None, "shear", "mirror", "nonuniform")      # instance i gets entry i % 5; None: left as it is
FLAT_AXIS = 1                                        # the local coordinate diag(1, 0, 1) makes constant
FLAT_OFF = 0.3
CLASSES = ("uniform2", "uniform_half", "tiny", "nonuniform", "mirror", "shear", "mixed", "flat_on", "flat_off")
ORACLE_CLASSES = tuple(c for c in CLASSES if not c.startswith("flat"))      # flat: every triangle of a mesh in one plane, coplanar ties
NONRIGID = tuple(c for c in CLASSES if c != "mirror")                         # a reflection is orthogonal: the length queries take it
CELL_MAX = 2.0 ** 10


def base_scene(name):
    """The golden scene at 64 x 48: the camera's pixel axes stretched so that the frame keeps the golden's field of view."""
    sc = copy.deepcopy(util.load_golden("cube" if name == "cube" else "materials_aniso")[0])
    w0, h0 = int(sc.config["width"][0]), int(sc.config["height"][0])
    sc.config["width"] = WIDTH; sc.config["height"] = HEIGHT
    cam = sc.camera.copy()
    cam["rotated_x_axis"] = (cam["rotated_x_axis"].astype(f64) * (w0 / WIDTH)).astype(f32)
    cam["rotated_y_axis"] = (cam["rotated_y_axis"].astype(f64) * (h0 / HEIGHT)).astype(f32)
    sc.camera = cam
    return sc


def mat4(cells):
    return np.asarray(cells, f64).reshape(4, 4)


def lift(L):
    m = np.eye(4); m[:3, :3] = L
    return m


def node_planes(blas, axis):
    """Every finite box-plane coordinate of the BLAS on that axis, float32, sorted."""
    c = np.concatenate([blas.nodes["aabb_min"][:, axis], blas.nodes["aabb_max"][:, axis]]).astype(f32)
    return np.unique(c[np.isfinite(c)])


def plane_member(sc, i):
    """The constant local coordinate of a flattened instance (the translation cell of world_inv's zero row) lies exactly on a box plane."""
    wi = np.asarray(sc.instances["world_inv"][i], f32).reshape(4, 4)
    return bool(np.any(node_planes(sc.blas[int(sc.instances["blas_id"][i])], FLAT_AXIS) == wi[FLAT_AXIS, 3]))


def corner_box(world64, root):
    """float64 box of the eight corners of the BLAS root box through the world matrix, padded by 1e-5 of its size (sideset.world_box)."""
    lo, hi = np.asarray(root["aabb_min"], f64), np.asarray(root["aabb_max"], f64)
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
    q = corners @ world64[:3, :3].T + world64[:3, 3]
    mn, mx = q.min(0), q.max(0)
    pad = 1e-5 * float((mx - mn).max()) + 1e-6
    return mn - pad, mx + pad


def with_linear(sc, Ls, flat_constant=None):
    """A copy of sc with instance i's matrices multiplied by Ls[i % len(Ls)] (None: that instance stays as it is).  flat_constant: for
    instances flattened by a singular L, "on" puts the constant local coordinate on the box plane of the instance's BLAS nearest the
    middle of its root box among those that are not 0 (membership asserted), a float puts it there."""
    from pyrtx import host
    sc = copy.deepcopy(sc)
    inst = sc.instances.copy()
    n = len(inst)
    aabbs = np.zeros((n, 6), f32); centres = np.zeros((n, 3), f32)
    for i in range(n):
        L = Ls[i % len(Ls)]
        blas = sc.blas[int(inst["blas_id"][i])]
        w, wi = mat4(inst["world"][i]), mat4(inst["world_inv"][i])
        if L is not None:
            L = np.asarray(L, f64)
            w = w @ lift(L); wi = lift(np.linalg.pinv(L)) @ wi
            if abs(np.linalg.det(L)) == 0.0:
                assert not wi[FLAT_AXIS].any(), "diag(1, 0, 1): a zero row in world_inv, translation cell included"
                if flat_constant == "on":
                    planes = node_planes(blas, FLAT_AXIS)
                    planes = planes[planes != 0]                      # a constant of exactly 0 is left out (Non-rigid matrices)
                    root = blas.nodes[0]
                    mid = 0.5 * (float(root["aabb_min"][FLAT_AXIS]) + float(root["aabb_max"][FLAT_AXIS]))
                    wi[FLAT_AXIS, 3] = float(planes[np.argmin(np.abs(planes.astype(f64) - mid))])
                else:
                    wi[FLAT_AXIS, 3] = float(f32(flat_constant))
        inst["world"][i] = w.astype(f32).reshape(16); inst["world_inv"][i] = wi.astype(f32).reshape(16)
        mn, mx = corner_box(mat4(inst["world"][i]), blas.nodes[0])
        aabbs[i, :3] = np.nextafter(mn.astype(f32), f32(-np.inf)); aabbs[i, 3:] = np.nextafter(mx.astype(f32), f32(np.inf))
        centres[i] = inst["world"][i].reshape(4, 4)[:3, 3]
    sc.instances = inst
    sc.tlas_nodes, sc.tlas_indices = host.tlas_build_balanced(centres, aabbs)
    if flat_constant == "on":
        assert all(plane_member(sc, i) for i in range(n))
    return sc


@functools.lru_cache(maxsize=None)
def _scene(base, cls):
    sc = base_scene(base)
    if cls == "mixed":
        return with_linear(sc, [None if k is None else LINEAR[k] for k in MIXED])
    if cls == "flat_on":
        return with_linear(sc, [LINEAR["flat"]], "on")
    if cls == "flat_off":
        return with_linear(sc, [LINEAR["flat"]], FLAT_OFF)
    return with_linear(sc, [LINEAR[cls]])


def scene(base, cls):
    """The base scene ("cube", "materials") under the class; a fresh copy, so that a test may change it."""
    return copy.deepcopy(_scene(base, cls))


def triangles_only(sc):
    """The scene without its spheres and planes: what the float64 triangle reference describes."""
    from pyrtx import scene_io as sio
    sc = copy.deepcopy(sc)
    sc.spheres = np.zeros(0, sio.SPHERE); sc.planes = np.zeros(0, sio.PLANE)
    return sc


# ---- the plain float64 reference: Moeller-Trumbore in world space over the triangles moved by the float64 world matrix ------------------------
RAY_EPSILON = 0.005


def world_triangles(sc):
    """-> (p0, e1, e2 (T, 3) float64 in world space, instance (T,), slot (T,)): every triangle slot of every instance through its world matrix."""
    P0, E1, E2, owner, slot = [], [], [], [], []
    for i in range(len(sc.instances)):
        hot = sc.blas[int(sc.instances["blas_id"][i])].tri_hot
        w = mat4(sc.instances["world"][i])
        A = w[:3, :3]
        P0.append(hot["position_0"].astype(f64) @ A.T + w[:3, 3])
        E1.append(hot["position_edge_1"].astype(f64) @ A.T); E2.append(hot["position_edge_2"].astype(f64) @ A.T)
        owner.append(np.full(len(hot), i)); slot.append(np.arange(len(hot)))
    return np.concatenate(P0), np.concatenate(E1), np.concatenate(E2), np.concatenate(owner), np.concatenate(slot)


def canonical_slots(blas):
    """slot -> the lowest slot of the BLAS with the same hot record bit for bit: a tree whose leaves share triangles (the reference's SBVH)
    holds such a triangle once per slot, and which of the identical slots wins is no difference in geometry."""
    rec = np.ascontiguousarray(blas.tri_hot).view(np.uint8).reshape(len(blas.tri_hot), -1)
    _, first, inverse = np.unique(rec, axis=0, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)]


def trace64(tris, rays6):
    """Two-sided Moeller-Trumbore of every ray against every triangle in float64, the reference's acceptance rules (0 < u, 0 < v, u + v < 1,
    t > RAY_EPSILON) -> (t (n,) of the nearest hit or inf, its index into tris or -1, t of the runner-up or inf)."""
    p0, e1, e2, _, _ = tris
    o = np.asarray(rays6, f64)[:, None, :3]; d = np.asarray(rays6, f64)[:, None, 3:6]
    with np.errstate(all="ignore"):
        h = np.cross(d, e2[None])
        a = (e1[None] * h).sum(2)
        f = 1.0 / a
        s = o - p0[None]
        u = f * (s * h).sum(2)
        q = np.cross(s, e1[None])
        v = f * (d * q).sum(2)
        t = f * (e2[None] * q).sum(2)
        ok = (u > 0) & (u < 1) & (v > 0) & (u + v < 1) & (t > RAY_EPSILON) & np.isfinite(t)
    t = np.where(ok, t, np.inf)
    order = np.argsort(t, axis=1)[:, :2]
    rows = np.arange(len(t))
    best = t[rows, order[:, 0]]
    second = t[rows, order[:, 1]] if t.shape[1] > 1 else np.full(len(t), np.inf)
    return best, np.where(np.isfinite(best), order[:, 0], -1), second


def aimed_rays(sc, count, seed):
    """count rays from outside the box of the world-space triangles, each aimed at the point of barycentrics (u, v) in [0.1, 0.4]^2 of a
    random triangle -> (count, 6) float32, directions of unit length before the rounding."""
    rng = np.random.default_rng(seed)
    p0, e1, e2, _, _ = world_triangles(sc)
    verts = np.concatenate([p0, p0 + e1, p0 + e2])
    lo, hi = verts.min(0), verts.max(0)
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    t = rng.integers(0, len(p0), count)
    uv = rng.uniform(0.1, 0.4, (count, 2))
    target = p0[t] + uv[:, :1] * e1[t] + uv[:, 1:] * e2[t]
    v = rng.normal(size=(count, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    # outside the sphere around the box, and at least 0.05 away: the reference accepts no hit nearer than RAY_EPSILON
    origin = (centre + v * (radius * rng.uniform(1.5, 3.0, (count, 1)) + 0.05)).astype(f32)
    assert np.all(np.any((origin < lo) | (origin > hi), axis=1))
    d = target - origin.astype(f64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([origin, d.astype(f32)], axis=1)


# ---- the safety condition of every row a GPU test sends ----------------------------------------------------------------------------------------
def xform_pos32(c, p):
    """csrc/rtx_math.h xform_pos in numpy float32, its order of operations: c[0] * x + (c[1] * y + (c[2] * z + c[3])) per row."""
    c = np.asarray(c, f32).reshape(4, 4); p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        return np.stack([c[a, 0] * p[..., 0] + (c[a, 1] * p[..., 1] + (c[a, 2] * p[..., 2] + c[a, 3])) for a in range(3)], -1).astype(f32)


def xform_dir32(c, d):
    c = np.asarray(c, f32).reshape(4, 4); d = np.asarray(d, f32)
    with np.errstate(all="ignore"):
        return np.stack([c[a, 0] * d[..., 0] + (c[a, 1] * d[..., 1] + c[a, 2] * d[..., 2]) for a in range(3)], -1).astype(f32)


def matrices_safe(sc):
    """Every cell of every instance matrix is finite and at most 2^10 in magnitude."""
    m = np.concatenate([sc.instances["world"].reshape(-1), sc.instances["world_inv"].reshape(-1)]).astype(f64)
    return bool(np.all(np.isfinite(m)) and np.all(np.abs(m) <= CELL_MAX))


def rows_safe(sc, origins, directions=None):
    """The local origin (and direction) of every row in every instance, and the row itself, are finite float32: no row of these reaches the
    case csrc/rtx_trace.h describes above ray_is_finite (a non-finite local origin under a finite direction)."""
    o = np.asarray(origins, f32)
    ok = np.all(np.isfinite(o))
    d = None if directions is None else np.asarray(directions, f32)
    if d is not None:
        ok = ok and np.all(np.isfinite(d))
    for i in range(len(sc.instances)):
        ok = ok and np.all(np.isfinite(xform_pos32(sc.instances["world_inv"][i], o))) and np.all(np.isfinite(xform_pos32(sc.instances["world"][i], o)))
        if d is not None:
            ok = ok and np.all(np.isfinite(xform_dir32(sc.instances["world_inv"][i], d))) and np.all(np.isfinite(xform_dir32(sc.instances["world"][i], d)))
    return bool(ok)


# ---- the rows the GPU tests send (tests/test_gpu_affine.py), built once and checked by tests/test_affine_cpu.py first -----------------------------
PER_CLASS = 56                                       # rayset classes x this <= 448 rows per set
SEED = 41
# materials under `tiny` is left to the CPU: world_inv = 2^10 . world_inv carries the instances' positions (up to 9 units) into cells of
# up to 9216, beyond the 2^10 every matrix a GPU test sends must respect (matrices_safe); cube under `tiny` has cells of exactly 2^10
UNSAFE = (("materials", "tiny"),)
GPU_SETS = tuple((b, c) for b in BASES for c in CLASSES if (b, c) not in UNSAFE)


def camera_rows(sc, cameras=None):
    """(origins, directions) of the primary rays of the scene's camera (or of `cameras`): d = x_axis * i + (y_axis * j + top_left)."""
    cams = sc.camera if cameras is None else cameras
    j, i = np.meshgrid(np.arange(sc.height, dtype=f32), np.arange(sc.width, dtype=f32), indexing="ij")
    o, d = [], []
    for cam in cams:
        ax, ay, tl = (np.asarray(cam[k], f32) for k in ("rotated_x_axis", "rotated_y_axis", "rotated_top_left_corner"))
        dd = ax * i.reshape(-1, 1) + (ay * j.reshape(-1, 1) + tl)
        d.append(dd); o.append(np.broadcast_to(np.asarray(cam["position"], f32), dd.shape))
    return np.concatenate(o), np.concatenate(d)


def traceable(sc):
    """test_gpu_rays.traceable: the debug hooks need a level-1 ray queue and a light; neither changes what a ray hits."""
    from pyrtx import scene_io as sio
    sc = copy.deepcopy(sc)
    sc.config["bounces"] = max(1, int(sc.config["bounces"][0]))
    if len(sc.point_lights) + len(sc.spot_lights) + len(sc.dir_lights) == 0:
        pl = np.zeros(1, sio.POINT_LIGHT); pl["colour"] = 1.0; pl["position"] = (0.0, 5.0, 0.0)
        sc.point_lights = pl
    return sc


@functools.lru_cache(maxsize=None)
def ray_rows(base, cls):
    """(scene, rays18 (N <= 448, 18), distances (N, 7), labels, oracle hits (N, 27), oracle ids (N, 3), oracle occlusion (N, 7)): the
    adversarial ray classes of tests/rayset.py over the scene and one more, `aimed` (aimed_rays: a shrunken mesh is hit by few of the
    others), once per run.  The rays of the class `far` start at |o| ~ 1e6: under `tiny` their local origins reach 2^30, finite."""
    import orc
    import rayset
    sc = traceable(scene(base, cls))
    o = orc.OracleScene(sc)
    rays, _, labels, _ = rayset.generate(sc, PER_CLASS, SEED, o)
    rng = np.random.default_rng(SEED)
    aimed = np.concatenate([aimed_rays(sc, PER_CLASS, SEED), rayset._differentials(rng, PER_CLASS)], axis=1).astype(f32)
    rays = np.ascontiguousarray(np.concatenate([rays[:448 - PER_CLASS], aimed])); labels = np.concatenate([labels[:448 - PER_CLASS], np.full(PER_CLASS, "aimed")])
    hits, ids = o.trace_closest(rays)
    dist = rayset.all_distances(rayset.shadow_distances(hits[:, 1]))
    return sc, rays, dist, labels, hits, ids, o.trace_any(rays, dist)


RAY_CLASSES = ("incoherent", "box_planes", "tiny_dirs", "edges", "surface", "spheres_planes", "far", "aimed")      # rayset.CLASSES and `aimed`


def zero_diff(rays18):
    r = np.array(rays18, f32); r[:, 6:] = 0
    return r


def length_rows(sc, count=24, seed=5):
    """Rows of the five length queries near the scene: points (n, 4), sweeps (n, 8), boxes (n, 10), box sweeps (n, 14), float32."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(sc.tlas_nodes[0]["aabb_min"], f64), np.asarray(sc.tlas_nodes[0]["aabb_max"], f64)
    ext = np.maximum(hi - lo, 1e-3)
    p = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (count, 3))
    d = rng.normal(size=(count, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    q = rng.normal(size=(count, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    h = rng.uniform(0.05, 0.3, (count, 3)) * float(ext.max())
    size = float(ext.max())
    points = np.concatenate([p, np.full((count, 1), 2.0 * size)], 1).astype(f32)
    sweeps = np.concatenate([p, d, np.full((count, 1), 4.0 * size), rng.uniform(0.02, 0.2, (count, 1)) * size], 1).astype(f32)
    boxes = np.concatenate([p, h, q], 1).astype(f32)
    box_sweeps = np.concatenate([p, d, np.full((count, 1), 4.0 * size), h, q], 1).astype(f32)
    return points, sweeps, boxes, box_sweeps


# ---- the record of what the walks did with a scaled matrix before they refused it (tests/test_affine_cpu.py) -----------------------------------
def finding_scene():
    """The golden cube with its one instance enlarged by 2: world = diag(2), world_inv = diag(0.5), the TLAS leaf box scaled to match."""
    return with_linear(copy.deepcopy(util.load_golden("cube")[0]), [LINEAR["uniform2"]])


IDQ = (0.0, 0.0, 0.0, 1.0)
FINDING = {
    # query: (rows, what the walk twin answered before the refusal, what the exhaustive twin answers: distance, t or count)
    "nearest": (np.array([[6, .1, .2, 2.5], [3.2, .1, .2, .7]], f32), (np.inf, np.inf), (2.0, 0.6)),
    "sweep": (np.array([[6, 2.6, 0, -1, 0, 0, 100, .4]], f32), (np.inf,), (3.47,)),
    "overlap": (np.array([[2.6, 0, 0, .4, .4, .4, *IDQ]], f32), (0,), (2,)),
    "sweep_box": (np.array([[6, 2.6, 0, -1, 0, 0, 100, .4, .4, .4, *IDQ]], f32), (np.inf,), (2.40,)),
}
