"""Labelled point classes for nearest-point queries (Renderer.query_nearest / host.query_nearest), per scene, like rayset.py for rays:
  vertex / edge / face   exactly on a triangle (dyadic barycentric weights, so the local-space point is exact for small meshes)
  off_tiny / off_large   off a face along its normal by 1e-5 .. 1e-3 and by 0.1 .. 3 of the scene size, both sides
  bisector               on the bisector plane of two faces that share an edge: an exact tie where the arithmetic allows one
  box_plane              on a face of a BVH node's box (a box distance of exactly 0 on one axis, pruning ties)
  inside                 the middle of every mesh's root box (inside closed meshes)
  sphere_centre          the centre of every sphere (direction (0, 1, 0) by rule)
  uniform / far / huge   uniform in the scene box, 100 scene sizes away, 1e30
  hostile                NaN, +-inf and denormal coordinates
and the maximum distances of distance_rows(): +inf, NaN, 0, -0, negative, nextafter of the host's distance both ways, a tenth of it."""
import numpy as np

f32 = np.float32
CLASSES = ["vertex", "edge", "face", "off_tiny", "off_large", "bisector", "box_plane", "inside", "sphere_centre", "uniform", "far", "huge", "hostile"]


def _xform(m16, p):
    m = np.asarray(m16, np.float64).reshape(4, 4)
    return (np.asarray(p, np.float64) @ m[:3, :3].T + m[:3, 3]).astype(f32)


def world_box(sc):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i in np.asarray(sc.tlas_indices):
        b = sc.blas[int(sc.instances[i]["blas_id"])].nodes[0]
        corners = np.array([[b["aabb_min"][0] if k & 1 else b["aabb_max"][0], b["aabb_min"][1] if k & 2 else b["aabb_max"][1],
                             b["aabb_min"][2] if k & 4 else b["aabb_max"][2]] for k in range(8)])
        w = _xform(sc.instances[i]["world"], corners)
        lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
    for s in sc.spheres:
        r = np.sqrt(float(s["radius_squared"]))
        lo, hi = np.minimum(lo, s["center"] - r), np.maximum(hi, s["center"] + r)
    if not np.isfinite(lo).all():
        lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    return lo, hi


def _triangles(sc, rng, n):
    """n random (instance, slot) with finite vertices -> (instance matrices, p0, e1, e2)."""
    out = []
    insts = np.asarray(sc.tlas_indices)
    for _ in range(n):
        i = int(insts[rng.integers(len(insts))])
        hot = sc.blas[int(sc.instances[i]["blas_id"])].tri_hot
        t = int(rng.integers(len(hot)))
        out.append((sc.instances[i]["world"], hot["position_0"][t], hot["position_edge_1"][t], hot["position_edge_2"][t]))
    return out


def _shared_edges(hot, limit=400):
    """Pairs (t0, t1, a, b) of triangles among the first `limit` slots that share the edge (a, b) exactly."""
    m = min(len(hot), limit)
    v = np.stack([hot["position_0"][:m], hot["position_0"][:m] + hot["position_edge_1"][:m], hot["position_0"][:m] + hot["position_edge_2"][:m]], axis=1)
    edges = {}
    pairs = []
    for t in range(m):
        for k in range(3):
            a, b = v[t, k].tobytes(), v[t, (k + 1) % 3].tobytes()
            key = (a, b) if a < b else (b, a)
            if key in edges and edges[key] != t:
                pairs.append((edges[key], t, v[t, k], v[t, (k + 1) % 3]))
            else:
                edges[key] = t
    return pairs, v


def generate(sc, n=256, seed=0):
    """-> (points float32 (N, 4) with maximum distance +inf, labels int (N,) into CLASSES); about n points, every class present where the
    scene allows it."""
    rng = np.random.default_rng(seed)
    lo, hi = world_box(sc)
    size = float(np.max(hi - lo))
    per = max(4, n // 12)
    pts, lab = [], []

    def put(name, p):
        p = np.atleast_2d(np.asarray(p, f32))
        pts.append(p); lab.append(np.full(len(p), CLASSES.index(name)))

    if len(sc.tlas_indices):
        dyadic = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
        for k, (w, p0, e1, e2) in enumerate(_triangles(sc, rng, 3 * per)):
            kind = ("vertex", "edge", "face")[k % 3]
            if kind == "vertex":
                u, v = [(0, 0), (1, 0), (0, 1)][k // 3 % 3]
            elif kind == "edge":
                t = dyadic[1 + k // 3 % 3]
                u, v = [(t, 0), (0, t), (1 - t, t)][k // 9 % 3]
            else:
                u, v = [(0.25, 0.25), (0.5, 0.25), (0.125, 0.625)][k // 3 % 3]
            put(kind, _xform(w, p0.astype(np.float64) + u * e1.astype(np.float64) + v * e2.astype(np.float64)))
        for k, (w, p0, e1, e2) in enumerate(_triangles(sc, rng, 2 * per)):
            nrm = np.cross(e1.astype(np.float64), e2.astype(np.float64))
            ln = np.linalg.norm(nrm)
            if not ln > 0:
                continue
            nrm /= ln
            q = p0 + rng.uniform(0.05, 0.45) * e1 + rng.uniform(0.05, 0.45) * e2
            tiny = k % 2 == 0
            step = (10.0 ** rng.uniform(-5, -3) if tiny else rng.uniform(0.1, 3.0) * size) * (1 if k % 4 < 2 else -1)
            put("off_tiny" if tiny else "off_large", _xform(w, q + step * nrm))
        got = 0
        for i in np.asarray(sc.tlas_indices):
            inst = sc.instances[int(i)]
            pairs, v = _shared_edges(sc.blas[int(inst["blas_id"])].tri_hot)
            for (t0, t1, a, b) in pairs[:per]:
                n0 = np.cross(v[t0, 1] - v[t0, 0], v[t0, 2] - v[t0, 0]).astype(np.float64); n1 = np.cross(v[t1, 1] - v[t1, 0], v[t1, 2] - v[t1, 0]).astype(np.float64)
                if not (np.linalg.norm(n0) > 0 and np.linalg.norm(n1) > 0):
                    continue
                d = n0 / np.linalg.norm(n0) + n1 / np.linalg.norm(n1)
                mid = 0.5 * (a.astype(np.float64) + b.astype(np.float64))
                put("bisector", _xform(inst["world"], mid + rng.choice([-0.5, 0.25, 1.0]) * size * 0.1 * d)); got += 1
            if got >= per:
                break
        for _ in range(per):
            i = int(np.asarray(sc.tlas_indices)[rng.integers(len(sc.tlas_indices))])
            inst = sc.instances[i]
            nodes = sc.blas[int(inst["blas_id"])].nodes
            nd = nodes[int(rng.integers(len(nodes)))]
            if not (np.isfinite(nd["aabb_min"]).all() and np.isfinite(nd["aabb_max"]).all()):
                continue
            p = rng.uniform(nd["aabb_min"] - 0.2 * size, nd["aabb_max"] + 0.2 * size)
            a = int(rng.integers(3))
            p[a] = nd["aabb_min"][a] if rng.integers(2) else nd["aabb_max"][a]
            put("box_plane", _xform(inst["world"], p))
        for i in np.asarray(sc.tlas_indices)[:per]:
            inst = sc.instances[int(i)]
            b = sc.blas[int(inst["blas_id"])].nodes[0]
            put("inside", _xform(inst["world"], 0.5 * (b["aabb_min"].astype(np.float64) + b["aabb_max"])))
    for s in sc.spheres:
        put("sphere_centre", s["center"])
    put("uniform", rng.uniform(lo - 0.25 * size, hi + 0.25 * size, size=(2 * per, 3)))
    d = rng.normal(size=(per, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    put("far", 0.5 * (lo + hi) + 100.0 * size * d)
    put("huge", [[1e30, 0, 0], [-1e30, 1e30, 1e30], [3e38, 3e38, -3e38], [0, 1e20, 0]])
    mid = (0.5 * (lo + hi)).astype(f32)
    hostile = [[np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]], [mid[0], mid[1], -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan],
               [1e-42, -1e-42, 1e-45], [-0.0, 0.0, -0.0]]
    put("hostile", hostile)
    p = np.concatenate(pts).astype(f32)
    return np.ascontiguousarray(np.concatenate([p, np.full((len(p), 1), np.inf, f32)], axis=1)), np.concatenate(lab)


def distance_rows(points, host_distance):
    """The same points at the hostile and the critical maximum distances: NaN, 0, -0, -1, -inf, nextafter of the host's own distance
    (host_distance, float32 (N,), inf where there is no answer) down and up, and a tenth of it.  -> float32 (7 N + ..., 4)."""
    p = np.asarray(points, f32)[:, :3]
    d = np.asarray(host_distance, f32)
    cols = [np.full(len(p), v, f32) for v in (np.nan, 0.0, -0.0, -1.0, -np.inf)]
    cols += [np.nextafter(d, f32(-np.inf)), np.nextafter(d, f32(np.inf)), d * f32(0.1), d]
    return np.ascontiguousarray(np.concatenate([np.concatenate([p, c[:, None]], axis=1) for c in cols]).astype(f32))
