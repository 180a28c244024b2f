"""Labelled capsules for the capsule-overlap queries (rtx_query_overlap_capsule; csrc/rtx_capsule_math.h), seeded, for any scene the query walks.

generate(sc, n, seed) -> (rows float32 (N, 7) of (start point p, axis vector d, radius r), labels int (N,) into CLASSES).  Classes:
  far            far away from everything
  inside         inside the first instance's mesh, around the middle of its root box, small: touches nothing when that mesh is closed and hollow
  face / edge / vertex   the axis through, or near, that feature of a random triangle, at random directions
  along_edge     the axis nearly parallel to a triangle's edge (the ill-conditioned pair), beside it at a clear offset, r clearly below or above it
  in_plane       the axis nearly parallel to a triangle's plane, over its face at a clear height, r clearly below or above it
  pierce         r tiny or 0, the axis through a face's interior, well clear of the triangle's edges and with both end points well off the plane
  ball           d = 0: a ball over a face at a clear height, r clearly below or above it
  segment        r = 0, random segments around a triangle: through it or past it
  point          d = 0 and r = 0, off the surface by a clear offset
  object / scene containing one whole instance, or everything
  long_thin      many times the scene's size long, a thousandth of a triangle thick, through a face
  touch_face / touch_edge / touch_vertex / touch_vertex_off   exact touching, made only for a scene whose first instance is the unmoved golden
                 `cube` (the mesh [-1, 1]^3).  touch_face: an axis parallel to the face x = 1 at x = 1 + r, r a power of two; touch_edge: an axis
                 parallel to the edge x = y = 1 at (1 + 3 s, 1 + 4 s), r = 5 s; touch_vertex: the start point at (1, 1, 1) + (2, 3, 6) s with
                 r = 7 s and the axis leading away, s a power of two — the end point, the squared distance and r * r are all exact in fp32 (a
                 rounded d / |d| would not be): these overlap.  touch_vertex_off: touch_vertex with r one ulp smaller — the surface one ulp
                 farther: it does not overlap.
  dead           NaN, inf, a negative r
NON_TOUCHING names the classes whose clearance from every surface is at least 1e-2 of the local size by construction (or random): the classes
a test may demand equality with the exhaustive search on.  segment_triangle_distance() is the fp64 distance the header's MARGIN is checked
against."""
import numpy as np

import hitset

f32 = np.float32
CLASSES = ("far", "inside", "face", "edge", "vertex", "along_edge", "in_plane", "pierce", "ball", "segment", "point", "object", "scene", "long_thin",
           "touch_face", "touch_edge", "touch_vertex", "touch_vertex_off", "dead")
NON_TOUCHING = ("far", "inside", "face", "edge", "vertex", "along_edge", "in_plane", "pierce", "ball", "segment", "point", "object", "scene", "long_thin")
TOUCHING = ("touch_face", "touch_edge", "touch_vertex")
KAPPA_MAX = 1024.0                                                  # the header's 2^10


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _perp(rng, a):
    """A random unit vector at right angles to a (any unit vector for a zero or non-finite a: a pad triangle's edge)."""
    n = np.linalg.norm(a)
    if not (np.isfinite(n) and n > 0):
        return _unit(rng)
    a = a / n
    while True:
        v = _unit(rng)
        v = v - (v @ a) * a
        if np.linalg.norm(v) > 0.2:
            return v / np.linalg.norm(v)


def _world_triangle(sc, rng):
    inst, p0, e1, e2 = hitset._triangle(sc, rng)
    v = np.stack([p0, p0 + e1, p0 + e2])
    m = np.asarray(inst["world"], np.float64).reshape(4, 4)
    return v if np.array_equal(m, np.eye(4)) else hitset._xform(inst["world"], v)


def is_dead(rows):
    r = np.asarray(rows, np.float64)
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(r).all(axis=1) & (r[:, 6] >= 0))


def is_cube(sc):
    if not (len(sc.tlas_nodes) and len(sc.instances)):
        return False
    inst0 = sc.instances[0]
    b = sc.blas[int(inst0["blas_id"])]
    return (np.array_equal(np.asarray(inst0["world"], np.float64).reshape(4, 4), np.eye(4)) and np.array_equal(b.nodes[0]["aabb_min"], [-1, -1, -1])
            and len(b.tri_hot) == 12)


def generate(sc, n=12, seed=0):
    rng = np.random.default_rng(seed)
    rows, labels = [], []

    def add(name, p, d, r):
        rows.append(np.concatenate([np.asarray(p, np.float64), np.asarray(d, np.float64), [float(r)]])); labels.append(CLASSES.index(name))

    def through(name, q, direction, length, r):
        """A capsule whose axis passes through q, a random share of its length on either side."""
        t = rng.uniform(0.3, 0.7)
        add(name, q - direction * length * t, direction * length, r)

    lo, hi = hitset.world_box(sc)
    ext = hi - lo
    has_tris = len(sc.tlas_nodes) > 0 and len(sc.instances) > 0
    for k in range(n):
        add("far", hi + ext * (2.0 + rng.uniform(0, 1, 3)) * np.where(rng.uniform(size=3) < 0.5, -1.0, 1.0) - np.where(k % 2, ext * 6, 0), _unit(rng) * rng.uniform(0.05, 0.5) * ext.min(),
            rng.uniform(0.05, 0.3) * ext.min())
        c = 0.5 * (lo + hi) + rng.uniform(-0.1, 0.1, 3) * ext
        d = _unit(rng) * rng.uniform(0.0, 0.5) * np.linalg.norm(ext) * (k % 2)
        add("scene", c - 0.5 * d, d, np.linalg.norm(ext) * rng.uniform(1.5, 2.5))
    if has_tris:
        inst0 = sc.instances[0]
        root = sc.blas[int(inst0["blas_id"])].nodes[0]
        rlo, rhi = root["aabb_min"].astype(np.float64), root["aabb_max"].astype(np.float64)
        for k in range(n):
            c_l = 0.5 * (rlo + rhi) + rng.uniform(-0.12, 0.12, 3) * (rhi - rlo)
            d_l = _unit(rng) * rng.uniform(0.0, 0.12) * (rhi - rlo).min()
            m0 = np.asarray(inst0["world"], np.float64).reshape(4, 4)
            add("inside", hitset._xform(inst0["world"], c_l), m0[:3, :3] @ d_l, rng.uniform(0.02, 0.1) * (rhi - rlo).min())
            leaf = sc.instances[int(rng.integers(len(sc.instances)))]
            r = sc.blas[int(leaf["blas_id"])].nodes[0]
            corners = np.array([[(r["aabb_max"] if (j >> a) & 1 else r["aabb_min"])[a] for a in range(3)] for j in range(8)], np.float64)
            w = hitset._xform(leaf["world"], corners)
            half = 0.5 * np.linalg.norm(w.max(axis=0) - w.min(axis=0))
            d = _unit(rng) * half * rng.uniform(0.0, 0.5)
            add("object", 0.5 * (w.min(axis=0) + w.max(axis=0)) - 0.5 * d, d, half * rng.uniform(1.1, 1.4) + 0.05)
            v = _world_triangle(sc, rng)
            size = max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[0]), 1e-3)
            nrm = np.cross(v[1] - v[0], v[2] - v[0]); nl = np.linalg.norm(nrm)
            nrm = nrm / nl if nl > 0 else np.array([0.0, 0.0, 1.0])
            on_face = rng.dirichlet((2, 2, 2)) @ v
            side = 1.0 if k % 4 < 2 else -1.0
            through("face", on_face + nrm * rng.uniform(-0.03, 0.03) * size, _unit(rng), rng.uniform(0.3, 1.2) * size, rng.uniform(0.05, 0.25) * size)
            e = int(rng.integers(3))
            on_edge = v[e] + (v[(e + 1) % 3] - v[e]) * rng.uniform(0.1, 0.9)
            through("edge", on_edge + rng.uniform(-0.02, 0.02, 3) * size, _unit(rng), rng.uniform(0.3, 1.2) * size, rng.uniform(0.05, 0.25) * size)
            through("vertex", v[e] + rng.uniform(-0.02, 0.02, 3) * size, _unit(rng), rng.uniform(0.3, 1.2) * size, rng.uniform(0.05, 0.25) * size)
            # along_edge: beside the edge at offset h, turned off it by 1e-3 .. 1e-2; r = h / 2 or 3 h / 2
            f = v[(e + 1) % 3] - v[e]
            fl = max(np.linalg.norm(f), 1e-6)
            off = _perp(rng, f)
            h = rng.uniform(0.05, 0.2) * size
            axis = f / fl + _perp(rng, f) * 10.0 ** rng.uniform(-3, -2)
            through("along_edge", v[e] + 0.5 * f + off * h, axis / np.linalg.norm(axis), rng.uniform(0.4, 1.5) * fl, h * (0.5 if k % 2 else 1.5))
            # in_plane: over the face at height h, tilted out of the plane by 1e-3
            h = rng.uniform(0.05, 0.2) * size
            axis = _perp(rng, nrm) + nrm * 1e-3 * (1 if k % 3 else -1)
            through("in_plane", on_face + nrm * h * side, axis / np.linalg.norm(axis), rng.uniform(0.2, 0.8) * size, h * (0.5 if k % 2 else 1.5))
            # pierce: through the face's interior, within 60 degrees of the normal, both ends well off the plane
            inner = rng.dirichlet((6, 6, 6)) @ v
            axis = nrm + _perp(rng, nrm) * rng.uniform(0.0, 1.5)
            through("pierce", inner, axis / np.linalg.norm(axis), rng.uniform(0.5, 1.5) * size, 0.0 if k % 2 else 1e-4 * size)
            h = rng.uniform(0.05, 0.3) * size
            add("ball", on_face + nrm * h * side, (0.0, 0.0, 0.0), h * (0.5 if k % 2 else 1.5))
            q = on_face + (_unit(rng) * rng.uniform(0.3, 0.8) * size if k % 3 == 0 else 0.0)
            through("segment", q, _unit(rng), rng.uniform(0.3, 1.5) * size, 0.0)
            add("point", on_face + nrm * (0.05 + rng.uniform(0, 0.2)) * size * side, (0.0, 0.0, 0.0), 0.0)
            through("long_thin", on_face, _unit(rng), 10.0 * np.linalg.norm(ext), 1e-3 * size)
        if is_cube(sc):
            for k in range(n):                                           # every number is exact in fp32, and so is every sum the tests form
                r = 0.125 * (1 << (k % 3))
                add("touch_face", (1.0 + r, 0.25 * (k % 4) - 0.5, 0.125 * (k % 7) - 0.25), (0.0, 0.25 * (1 + k % 3), 0.125 * (k % 5) - 0.25), r)
                s = 0.03125 * (1 << (k % 3))
                add("touch_edge", (1.0 + 3 * s, 1.0 + 4 * s, 0.25 * (k % 5) - 0.75), (0.0, 0.0, 0.25 * (1 + k % 4)), 5 * s)
                p = (1.0 + 2 * s, 1.0 + 3 * s, 1.0 + 6 * s)
                d = (0.25 * (1 + k % 2), 0.125 * (k % 3), 0.5)
                add("touch_vertex", p, d, 7 * s)
                add("touch_vertex_off", p, d, np.nextafter(f32(7 * s), f32(0)))
    for k in range(n):
        p, d, r = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(0.1, 1)
        kind = k % 6
        if kind == 0: p[k % 3] = np.nan
        elif kind == 1: d[k % 3] = np.inf
        elif kind == 2: r = -0.125
        elif kind == 3: r = np.nan
        elif kind == 4: r = np.inf
        else: p[k % 3] = -np.inf
        add("dead", p, d, r)
    with np.errstate(over="ignore"):
        return np.array(rows).astype(f32), np.array(labels)


def in_classes(labels, names):
    return np.isin(labels, [CLASSES.index(c) for c in names])


def _point_segment(q, a, f):
    """fp64 distances from points q (T, 3) to the segments a + t f (T, 3 each)."""
    ff = np.einsum("tk,tk->t", f, f)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ff > 0, np.einsum("tk,tk->t", q - a, f) / np.where(ff > 0, ff, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(q - (a + f * t[:, None]), axis=1)


def _point_triangle(q, e1, e2):
    """fp64 distances from points q (T, 3), relative to each triangle's first vertex, to the triangles (0, e1, e2)."""
    zero = np.zeros_like(e1)
    best = np.minimum(np.minimum(_point_segment(q, zero, e1), _point_segment(q, zero, e2)), _point_segment(q, e1, e2 - e1))
    n = np.cross(e1, e2)
    nn = np.einsum("tk,tk->t", n, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = nn > 0
        nns = np.where(ok, nn, 1.0)
        u = np.einsum("tk,tk->t", np.cross(q, e2), n) / nns
        v = np.einsum("tk,tk->t", np.cross(e1, q), n) / nns
        inside = ok & (u >= 0) & (v >= 0) & (u + v <= 1)
        plane = np.abs(np.einsum("tk,tk->t", q, n)) / np.sqrt(nns)
    return np.where(inside, np.minimum(plane, best), best)


def _segment_segment(w, d, f):
    """fp64 distances between the segments w + s d and t f (T, 3 each; w relative to the second segment's start), and their kappa."""
    a, e = np.einsum("tk,tk->t", d, d), np.einsum("tk,tk->t", f, f)
    b, c, g = np.einsum("tk,tk->t", d, f), np.einsum("tk,tk->t", d, w), np.einsum("tk,tk->t", f, w)
    cr = np.linalg.norm(np.cross(d, f), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        kappa = np.where(cr > 0, np.sqrt(a * e) / np.where(cr > 0, cr, 1.0), np.inf)
        den = a * e - b * b
        ok = (den > 0) & (kappa < 1e7)
        s = np.where(ok, (b * g - c * e) / np.where(ok, den, 1.0), 0.0)
        t = np.where(ok, (a * g - b * c) / np.where(ok, den, 1.0), 0.0)
    interior = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    di = np.linalg.norm(w + d * s[:, None] - f * t[:, None], axis=1)
    ends = np.minimum(np.minimum(_point_segment(w, np.zeros_like(f), f), _point_segment(w + d, np.zeros_like(f), f)),
                      np.minimum(_point_segment(-w, np.zeros_like(d), d), _point_segment(f - w, np.zeros_like(d), d)))      # the edge's ends, relative to the segment's start
    return np.where(interior, np.minimum(di, ends), ends), kappa


def segment_triangle_distance(row, inst, hot):
    """One live row against every triangle of one instance, in fp64: (dist (T,), kappas (T, 4), S (T,), W, depth (T,), miss (T,)).
    dist: the exact distance from the segment to the triangle (0 when it pierces); kappas: the conditioning of the three edge pairs
    |d||f| / |d x f| (inf for a parallel pair, 1 for a ball) and of the piercing quotient |d||e1||e2| / |det|, as MARGIN defines them;
    S = |m| + |d| + |e1| + |e2| + r; W = |p| + |p_l|, 0 for an identity matrix; depth: where the segment pierces, how far the crossing point lies
    inside the triangle and the nearer end point off its plane, whichever is less (0 where it does not pierce) — what decides a row of r = 0;
    miss: where it does not pierce, by how much: the larger of the nearer end point's distance from the plane when both lie on one side, and
    the distance from the triangle of the point where the segment's LINE crosses the plane (inf for a ball or a line parallel to the plane) —
    the piercing test reports only if all its conditions hold, so this is what it would have to be wrong by."""
    r = np.asarray(row, np.float64)
    M = np.asarray(inst["world_inv"], np.float64).reshape(4, 4)
    p_l, d = M[:3, :3] @ r[:3] + M[:3, 3], M[:3, :3] @ r[3:6]
    W = 0.0 if np.array_equal(M, np.eye(4)) else float(np.linalg.norm(r[:3]) + np.linalg.norm(p_l))
    p0, e1, e2 = (np.asarray(hot[k], np.float64) for k in ("position_0", "position_edge_1", "position_edge_2"))
    T = len(p0)
    m = p_l - p0
    D = np.broadcast_to(d, (T, 3))
    dl = np.linalg.norm(d)
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    S = np.linalg.norm(m, axis=1) + dl + l1 + l2 + r[6]
    kappas = np.ones((T, 4))
    dist = _point_triangle(m, e1, e2)
    depth = np.zeros(T)
    miss = np.full(T, np.inf)
    if dl > 0:
        dist = np.minimum(dist, _point_triangle(m + D, e1, e2))
        for j, (q, f) in enumerate(((np.zeros_like(e1), e1), (np.zeros_like(e1), e2), (e1, e2 - e1))):
            dj, kj = _segment_segment(m - q, D, f)
            dist = np.minimum(dist, dj); kappas[:, j] = kj
        n = np.cross(e1, e2)
        det = -np.einsum("tk,tk->t", D, n)
        with np.errstate(invalid="ignore", divide="ignore"):
            kappas[:, 3] = np.where(det != 0, dl * l1 * l2 / np.where(det != 0, np.abs(det), 1.0), np.inf)
            nl = np.linalg.norm(n, axis=1)
            ok = (nl > 0) & (det != 0)
            sa = np.einsum("tk,tk->t", m, n) / np.where(ok, nl, 1.0)
            sb = np.einsum("tk,tk->t", m + D, n) / np.where(ok, nl, 1.0)
            t = np.where(ok, sa / np.where(sa != sb, sa - sb, 1.0), 0.0)
            x = m + D * t[:, None]
            nn = np.where(ok, nl * nl, 1.0)
            u = np.einsum("tk,tk->t", np.cross(x, e2), n) / nn
            v = np.einsum("tk,tk->t", np.cross(e1, x), n) / nn
            pierces = ok & (sa * sb < 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        zero = np.zeros_like(e1)
        rim = np.minimum(np.minimum(_point_segment(x, zero, e1), _point_segment(x, zero, e2)), _point_segment(x, e1, e2 - e1))
        dist = np.where(pierces, 0.0, dist)
        depth = np.where(pierces, np.minimum(rim, np.minimum(np.abs(sa), np.abs(sb))), 0.0)
        with np.errstate(invalid="ignore"):
            one_side = sa * sb >= 0
            miss = np.where(~ok, np.inf, np.where(pierces, 0.0, np.maximum(np.where(one_side, np.minimum(np.abs(sa), np.abs(sb)), 0.0), _point_triangle(x, e1, e2))))
    return dist, kappas, S, W, depth, miss
