"""Labelled row classes for swept-sphere queries (Renderer.query_sweep / host.query_sweep), per scene, like pointset.py and hitset.py.  A row
is (origin, direction, max distance D, radius r).  The head-on classes are built from a contact point on a triangle and an outward direction
there, so the feature the ball meets on THAT triangle is known by construction (another triangle of the mesh may still be met first):
  face_on / edge_on / vertex_on   head-on at a face point, an edge point, a vertex, from 0.5 .. 3 scene sizes away
  graze                           past an edge point at a closest approach of r (1 -+ 1e-3)
  far_small                       origin 10^3 and 10^4 radii away from a face point, r = 1e-2 and 1e-3 of the scene size
  overlap_deep / overlap_shallow  the centre 0.1 r and r (1 - 1e-4) off a face point at t = 0
  parallel_face                   moving parallel to a face at height r (1 -+ 1e-3)
  along_edge                      moving along an edge's line at 0.5 r and 1.5 r from it
  inside_sphere                   from inside every scene sphere, r a tenth of and nearly its radius
  plane_slab                      towards and away from every plane, inside its slab of +-r and outside it
  box_plane                       origin on a plane of a BVH node's box grown by r, moving along that plane
  miss / uniform                  away from the scene (a plane may still be met); uniform origins, directions and radii
  fat                             a ball of 0.5 .. 2 scene sizes from 4 .. 6 sizes away: every box is entered, the deepest stacks
  hostile                         NaN, inf, denormal and zero components, r in {0, -0, -1, NaN, inf}
and bound_rows(): the same rows at D = nextafter of the host's own t both ways, and at t itself."""
import numpy as np

import pointset

f32 = np.float32
CLASSES = ["face_on", "edge_on", "vertex_on", "graze", "far_small", "overlap_deep", "overlap_shallow", "parallel_face", "along_edge", "inside_sphere",
           "plane_slab", "box_plane", "miss", "uniform", "fat", "hostile"]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _any_perp(v, rng):
    while True:
        p = np.cross(v, rng.normal(size=3))
        if np.linalg.norm(p) > 1e-3 * np.linalg.norm(v):
            return _unit(p)


def is_live(rows):
    rows = np.asarray(rows, f32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(rows[:, :6]).all(axis=1) & (rows[:, 3:6] != 0).any(axis=1) & (rows[:, 6] > 0) & np.isfinite(rows[:, 7]) & (rows[:, 7] > 0))


def generate(sc, n=256, seed=0):
    """-> (rows float32 (N, 8), labels int (N,) into CLASSES); about n rows, every class present where the scene allows it."""
    rng = np.random.default_rng(seed)
    lo, hi = pointset.world_box(sc)
    size = float(np.max(hi - lo))
    mid = 0.5 * (lo + hi)
    per = max(3, n // 16)
    rows, lab = [], []

    def put(name, o, d, D, r):
        rows.append(np.concatenate([np.asarray(o, np.float64), np.asarray(d, np.float64), [D, r]])); lab.append(CLASSES.index(name))

    def world(w, p, d):
        m = np.asarray(w, np.float64).reshape(4, 4)
        return m[:3, :3] @ p + m[:3, 3], m[:3, :3] @ d

    tris = pointset._triangles(sc, rng, 12 * per) if len(sc.tlas_indices) else []
    k = 0
    for (w, p0, e1, e2) in tris:
        p0, e1, e2 = (x.astype(np.float64) for x in (p0, e1, e2))
        nrm = np.cross(e1, e2)
        if not (np.isfinite(nrm).all() and np.linalg.norm(nrm) > 0):
            continue
        nrm = _unit(nrm) * (1 if k % 2 else -1)
        cen = p0 + (e1 + e2) / 3
        r = size * 10.0 ** rng.uniform(-3, -1)
        speed = 10.0 ** rng.uniform(-1, 1)
        L = size * rng.uniform(0.5, 3.0)
        corner = [(0, 0), (1, 0), (0, 1)][k // 12 % 3]
        a = p0 + corner[0] * e1 + corner[1] * e2                              # a vertex, and the edge that starts there
        e = [e1, e2 - e1, -e2][k // 12 % 3]
        q_face = p0 + rng.uniform(0.1, 0.4) * e1 + rng.uniform(0.1, 0.4) * e2
        q_edge = a + rng.uniform(0.1, 0.9) * e
        ehat = _unit(e) if np.linalg.norm(e) > 0 else _unit(e1)
        out_edge = q_edge - cen; out_edge = out_edge - ehat * (out_edge @ ehat)          # in the plane, across the edge, away from the triangle
        out_edge = _unit(out_edge) if np.linalg.norm(out_edge) > 0 else nrm
        kind = k % 12
        if kind == 0:
            o, d = q_face + nrm * (r + L), -nrm * speed; put("face_on", *world(w, o, d), np.inf, r)
        elif kind == 1:
            u = _unit(out_edge + rng.uniform(0.0, 1.0) * nrm); o, d = q_edge + u * (r + L), -u * speed; put("edge_on", *world(w, o, d), np.inf, r)
        elif kind == 2:
            u = _unit(_unit(a - cen) + rng.uniform(0.0, 1.0) * nrm); o, d = a + u * (r + L), -u * speed; put("vertex_on", *world(w, o, d), np.inf, r)
        elif kind == 3:
            u = _unit(out_edge + 0.5 * nrm); t = _unit(np.cross(u, ehat)); f = 1 + (1e-3 if k % 24 < 12 else -1e-3)
            o, d = q_edge + u * r * f - t * L, t * speed; put("graze", *world(w, o, d), np.inf, r)
        elif kind == 4:
            r = size * (1e-2 if k % 24 < 12 else 1e-3); L = r * (1e3 if k % 48 < 24 else 1e4)
            u = _unit(nrm + 0.3 * rng.normal(size=3)); o, d = q_face + u * L, -u * speed; put("far_small", *world(w, o, d), np.inf, r)
        elif kind == 5:
            o, d = q_face + nrm * 0.1 * r, _unit(rng.normal(size=3)) * speed; put("overlap_deep", *world(w, o, d), np.inf, r)
        elif kind == 6:
            o, d = q_face + nrm * r * (1 - 1e-4), _unit(rng.normal(size=3)) * speed; put("overlap_shallow", *world(w, o, d), np.inf, r)
        elif kind == 7:
            t = _any_perp(nrm, rng); f = 1 + (1e-3 if k % 24 < 12 else -1e-3)
            o, d = q_face + nrm * r * f - t * L, t * speed; put("parallel_face", *world(w, o, d), np.inf, r)
        elif kind == 8:
            u = _any_perp(ehat, rng); f = 0.5 if k % 24 < 12 else 1.5
            o, d = a - ehat * L + u * r * f, ehat * speed; put("along_edge", *world(w, o, d), np.inf, r)
        elif kind == 9:
            i = int(np.asarray(sc.tlas_indices)[rng.integers(len(sc.tlas_indices))]); inst = sc.instances[i]
            nodes = sc.blas[int(inst["blas_id"])].nodes; nd = nodes[int(rng.integers(len(nodes)))]
            if np.isfinite(nd["aabb_min"]).all() and np.isfinite(nd["aabb_max"]).all():
                p = rng.uniform(nd["aabb_min"] - 0.2 * size, nd["aabb_max"] + 0.2 * size)
                ax = int(rng.integers(3)); r32 = f32(r)
                p[ax] = f32(nd["aabb_min"][ax] - r32) if rng.integers(2) else f32(nd["aabb_max"][ax] + r32)
                d = rng.normal(size=3) * speed; d[ax] = 0.0 if k % 24 < 12 else -0.0
                put("box_plane", *world(inst["world"], p, d), np.inf, r32)
        elif kind == 10:
            u = _unit(rng.normal(size=3)); put("miss", mid + u * size * 2, u * speed, np.inf, r)
        else:
            o = rng.uniform(lo - 0.25 * size, hi + 0.25 * size); put("uniform", o, rng.normal(size=3) * speed, np.inf if k % 24 < 12 else size * rng.uniform(0.1, 2), r)
        k += 1
    for s in sc.spheres:
        R = np.sqrt(float(s["radius_squared"]))
        for f in (0.1, 0.999):
            put("inside_sphere", s["center"] + rng.uniform(-1, 1, 3) * R * 0.0005, _unit(rng.normal(size=3)) * 0.5, np.inf, R * f)
        put("inside_sphere", s["center"] + _unit(rng.normal(size=3)) * R * 0.5, rng.normal(size=3), np.inf, R * 0.25)
    for p in sc.planes:
        nrm = p["normal"].astype(np.float64); base = -float(p["distance"]) * nrm + _any_perp(nrm, rng) * size * 0.3
        r = size * 0.05
        for h, sign in ((0.5, -1), (0.5, 1), (-0.25, 1), (3.0, -1), (3.0, 1), (-2.0, 1)):
            put("plane_slab", base + nrm * h * r, sign * nrm + 0.3 * _any_perp(nrm, rng), np.inf, r)
    for _ in range(per):
        put("uniform", rng.uniform(lo - 0.25 * size, hi + 0.25 * size), rng.normal(size=3), np.inf, size * 10.0 ** rng.uniform(-3, -1))
        u = _unit(rng.normal(size=3)); put("miss", mid + u * size * 1.5, u, np.inf, size * 0.01)
    for j in range(per):
        u = _unit(rng.normal(size=3)); f = (0.5, 1.0, 2.0)[j % 3]
        put("fat", mid + u * size * (4 + f), -u + 0.2 * rng.normal(size=3), np.inf, size * f)
    m = mid.astype(f32); r = size * 0.01
    for o, d, D, rr in [([np.nan, m[1], m[2]], [0, 0, 1], np.inf, r), ([m[0], np.inf, m[2]], [0, 0, 1], np.inf, r), (m, [np.nan, 0, 1], np.inf, r), (m, [0, -np.inf, 1], np.inf, r),
                        (m - [0, 0, 2 * size], [0, 0, 0], np.inf, r), (m - [0, 0, 2 * size], [-0.0, 0, -0.0], np.inf, r), (m - [0, 0, 2 * size], [0, 0, 1e-42], 1e6, r),
                        (m - [0, 0, 2 * size], [1e-45, 0, 1], np.inf, r), ([1e-42, -1e-42, 1e-45], [0, 0, 1], np.inf, r), (m - [0, 0, 2 * size], [0, 0, 1], np.nan, r),
                        (m - [0, 0, 2 * size], [0, 0, 1], 0.0, r), (m - [0, 0, 2 * size], [0, 0, 1], -1.0, r), (m - [0, 0, 2 * size], [0, 0, 1], -np.inf, r)] + \
                       [(m - [0, 0, 2 * size], [0, 0, 1], np.inf, bad) for bad in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf)]:
        put("hostile", o, d, D, rr)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.array(rows).astype(f32)), np.array(lab)


def bound_rows(rows, host_t):
    """The same rows at the critical maximum distances: nextafter of the host's own t (host_t, float32 (N,), inf where there is no answer) down
    and up, and t itself (no answer: the upper end is strict).  -> float32 (3 N, 8)."""
    rows = np.asarray(rows, f32); t = np.asarray(host_t, f32)
    out = []
    for D in (np.nextafter(t, f32(-np.inf)), np.nextafter(t, f32(np.inf)), t):
        c = rows.copy(); c[:, 6] = D; out.append(c)
    return np.ascontiguousarray(np.concatenate(out))
