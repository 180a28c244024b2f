"""Seeded adversarial rays for the traversal kernels (plain numpy; the oracle supplies the hit distances the shadow distances and the
surface starts are derived from).

generate(sc, n, seed) -> (rays18 (N, 18) float32, max_dist3 (N, 3) float32, labels (N,) class names, hits (N, 27) float32: the oracle's
closest hits of the rays, orc_trace_closest's layout).  Columns of a ray: origin, direction,
dO_dx, dO_dy, dD_dx, dD_dy (rtx_debug_trace_rays / orc_trace_closest).  max_dist3: the closest-hit distance t and one ulp below and above it
(a miss: FLT_MAX, inf, inf); FIXED_DIST are four more shadow distances every ray is tested at.  Classes (n rays each, fewer where the scene
has no such geometry):
  incoherent     origins uniform in the inflated world box, directions uniform on the sphere
  box_planes     origins exactly on BLAS node planes (object space of identity-rotation instances, world origin chosen so that the
                 transform lands on the plane bit for bit) and on TLAS node planes; the direction is +-0 on that axis, -0.0 origins on
                 +0.0 planes where the plane is world space
  tiny_dirs      subnormal and +-0 direction components: inverse components of +-inf and huge finite ones
  edges          aimed at triangle vertices and edge midpoints in world space, half of them along a coordinate axis (exact cracks / ties)
  surface        starting at the fp32 hit point of an earlier ray, in a fresh direction (secondary-like)
  spheres_planes inside spheres; parallel to and inside (or one ulp off) axis-aligned planes
  far            origins at |o| ~ 1e6, aimed into the scene
"""
import numpy as np

f32 = np.float32
FLT_MIN = np.finfo(f32).tiny
FLT_MAX = np.finfo(f32).max
FIXED_DIST = np.array([0.0, FLT_MIN, 1e30, np.inf], f32)
CLASSES = ("incoherent", "box_planes", "tiny_dirs", "edges", "surface", "spheres_planes", "far")


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _xform(m16, p):
    """Mesh transform (world / world_inv: row-major 3x4 in 16 floats) applied in float64: targets only need to be near the geometry."""
    m = np.asarray(m16, np.float64).reshape(4, 4)
    return p @ m[:3, :3].T + m[:3, 3]


def _world_box(sc):
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


def _identity_rotation(inst):
    w = np.asarray(inst["world_inv"], f32).reshape(4, 4)[:3, :3]
    return np.array_equal(w, np.eye(3, dtype=f32))


def _exact_world_coord(p, c):
    """A float32 x with fl(x + c) == p (Mesh::trace's transform_position of an identity-rotation instance), or None."""
    x = f32(f32(p) - f32(c))
    for cand in (x, np.nextafter(x, f32(-np.inf)), np.nextafter(x, f32(np.inf))):
        if f32(cand + f32(c)) == f32(p):
            return cand
    return None


def _differentials(rng, n):
    return np.concatenate([rng.uniform(-0.01, 0.01, (n, 6)), rng.uniform(-0.002, 0.002, (n, 6))], axis=1).astype(f32)


def _box_plane_rays(sc, rng, n, lo, hi):
    out = []
    # BLAS planes through identity-rotation instances
    cands = [k for k, inst in enumerate(sc.instances) if _identity_rotation(inst)]
    tries = 0
    while cands and len(out) < n // 2 and tries < 50 * n:
        tries += 1
        k = cands[int(rng.integers(len(cands)))]
        inst = sc.instances[k]
        nodes = sc.blas[int(inst["blas_id"])].nodes
        node = nodes[int(rng.integers(len(nodes)))]
        if not np.all(np.isfinite(node["aabb_min"])) or np.any(node["aabb_min"] > node["aabb_max"]):
            continue
        ax = int(rng.integers(3))
        plane = node["aabb_min"][ax] if rng.random() < 0.5 else node["aabb_max"][ax]
        c = np.asarray(inst["world_inv"], f32).reshape(4, 4)[:3, 3]
        # object-space origin inside (or a little around) the node's box, on the plane; the other axes need not be exact
        oo = rng.uniform(node["aabb_min"] - 0.1, node["aabb_max"] + 0.1).astype(f32)
        wo = (oo - c).astype(f32)
        x = _exact_world_coord(plane, c[ax])
        if x is None:
            continue
        wo[ax] = x
        d = _unit(rng, 1)[0]
        d[ax] = f32(-0.0) if rng.random() < 0.5 else f32(0.0)
        out.append(np.concatenate([wo, d]))
    # TLAS planes, world space
    while len(sc.tlas_nodes) and len(out) < n:
        node = sc.tlas_nodes[int(rng.integers(len(sc.tlas_nodes)))]
        ax = int(rng.integers(3))
        plane = f32(node["aabb_min"][ax] if rng.random() < 0.5 else node["aabb_max"][ax])
        wo = rng.uniform(node["aabb_min"] - 0.5, node["aabb_max"] + 0.5).astype(f32)
        wo[ax] = f32(-0.0) if plane == 0 and rng.random() < 0.5 else plane
        d = _unit(rng, 1)[0]
        r = rng.random()
        d[ax] = f32(-0.0) if r < 0.4 else f32(0.0) if r < 0.8 else d[ax]        # mostly parallel to the plane; some cross it
        out.append(np.concatenate([wo, d]))
    return np.array(out, f32).reshape(-1, 6)


def _tiny_dir_rays(sc, rng, n, lo, hi):
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, FLT_MIN, -FLT_MIN, 1e-30, -1e-30], f32)
    o = rng.uniform(lo, hi, (n, 3)).astype(f32)
    d = _unit(rng, n)
    for i in range(n):
        axes = rng.choice(3, size=int(rng.integers(1, 3)), replace=False)
        d[i, axes] = tiny[rng.integers(len(tiny), size=len(axes))]
    return np.concatenate([o, d], axis=1)


def _vertex_targets(sc, rng, n):
    pts = []
    if not len(sc.instances):
        return np.zeros((0, 3))
    for _ in range(n):
        inst = sc.instances[int(rng.integers(len(sc.instances)))]
        hot = sc.blas[int(inst["blas_id"])].tri_hot
        t = hot[int(rng.integers(len(hot)))]
        p0 = t["position_0"].astype(np.float64); p1 = p0 + t["position_edge_1"]; p2 = p0 + t["position_edge_2"]
        p = [p0, p1, p2, (p0 + p1) / 2, (p1 + p2) / 2, (p0 + p2) / 2][int(rng.integers(6))]
        pts.append(_xform(inst["world"], p[None])[0])
    return np.array(pts)


def _edge_rays(sc, rng, n, lo, hi):
    tg = _vertex_targets(sc, rng, n)
    if not len(tg):
        return np.zeros((0, 6), f32)
    m = len(tg)
    o = rng.uniform(lo, hi, (m, 3))
    d = tg - o
    axial = rng.random(m) < 0.5                                        # along one axis: the two other coordinates pass the target exactly
    for i in np.nonzero(axial)[0]:
        ax = int(rng.integers(3)); sgn = 1.0 if rng.random() < 0.5 else -1.0
        o[i] = tg[i]; o[i, ax] -= sgn * (hi[ax] - lo[ax])
        d[i] = 0.0; d[i, ax] = sgn
    o = o.astype(f32); d = d.astype(f32)
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    d = (d / norm).astype(f32)
    return np.concatenate([o, d], axis=1)


def _sphere_plane_rays(sc, rng, n):
    out = []
    for _ in range(n // 2 if len(sc.spheres) else 0):
        s = sc.spheres[int(rng.integers(len(sc.spheres)))]
        r = np.sqrt(float(s["radius_squared"]))
        o = (s["center"] + _unit(rng, 1)[0] * r * rng.uniform(0, 0.95)).astype(f32)
        out.append(np.concatenate([o, _unit(rng, 1)[0]]))
    axial = [p for p in sc.planes if np.count_nonzero(p["normal"]) == 1]
    for _ in range(n - len(out) if axial else 0):
        p = axial[int(rng.integers(len(axial)))]
        ax = int(np.flatnonzero(p["normal"])[0])
        o = rng.uniform(-6, 6, 3).astype(f32)
        o[ax] = f32(-p["distance"] / p["normal"][ax])                 # exactly in the plane (n = +-1)
        k = rng.random()
        if k < 0.25:
            o[ax] = np.nextafter(o[ax], f32(np.inf))
        elif k < 0.5:
            o[ax] = np.nextafter(o[ax], f32(-np.inf))
        d = _unit(rng, 1)[0]
        d[ax] = f32(-0.0) if rng.random() < 0.5 else f32(0.0)
        out.append(np.concatenate([o, d]))
    return np.array(out, f32).reshape(-1, 6)


def _far_rays(sc, rng, n, lo, hi):
    c = (lo + hi) / 2
    o = (c + _unit(rng, n).astype(np.float64) * rng.uniform(0.5e6, 2e6, (n, 1))).astype(f32)
    tg = rng.uniform(lo, hi, (n, 3))
    d = tg - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return np.concatenate([o, d], axis=1)


def shadow_distances(t):
    """The closest-hit distance and one ulp either side (Scene::intersect_primitives accepts t < max_distance strictly)."""
    t = np.asarray(t, f32)
    return np.stack([np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf))], axis=1).astype(f32)


def generate(sc, n=256, seed=0, oracle=None, threads=8):
    """n rays per class (see the module doc).  oracle: an orc.OracleScene over sc (made here when None)."""
    if oracle is None:
        import orc
        oracle = orc.OracleScene(sc)
    rng = np.random.default_rng(seed)
    lo, hi = _world_box(sc)
    parts = {
        "incoherent": np.concatenate([rng.uniform(lo, hi, (n, 3)).astype(f32), _unit(rng, n)], axis=1),
        "box_planes": _box_plane_rays(sc, rng, n, lo, hi),
        "tiny_dirs": _tiny_dir_rays(sc, rng, n, lo, hi),
        "edges": _edge_rays(sc, rng, n, lo, hi),
    }
    # surface starts: the fp32 hit points of the rays so far, new directions
    so_far = np.concatenate(list(parts.values()))
    hits, _ = oracle.trace_closest(np.concatenate([so_far, np.zeros((len(so_far), 12), f32)], axis=1), threads)
    hp = hits[hits[:, 0] > 0, 2:5]
    pick = rng.integers(len(hp), size=min(n, len(hp))) if len(hp) else np.zeros(0, int)
    parts["surface"] = np.concatenate([hp[pick], _unit(rng, len(pick))], axis=1).astype(f32)
    parts["spheres_planes"] = _sphere_plane_rays(sc, rng, n)
    parts["far"] = _far_rays(sc, rng, n, lo, hi)
    od = np.concatenate([parts[k] for k in CLASSES]).astype(f32)
    labels = np.concatenate([np.full(len(parts[k]), k) for k in CLASSES])
    rays = np.concatenate([od, _differentials(rng, len(od))], axis=1).astype(f32)
    hits, _ = oracle.trace_closest(rays, threads)
    return rays, shadow_distances(hits[:, 1]), labels, hits


def all_distances(max_dist3):
    """(N, 7): the three per-ray distances, then FIXED_DIST."""
    return np.concatenate([max_dist3, np.broadcast_to(FIXED_DIST, (len(max_dist3), len(FIXED_DIST)))], axis=1).astype(f32)
