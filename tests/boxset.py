"""Labelled boxes for the box-overlap queries (rtx_query_overlap; csrc/rtx_overlap_math.h), seeded, for any scene the query walks.

generate(sc, n, seed) -> (boxes float32 (N, 10) of (centre, half extents, quaternion x y z w), labels int (N,) into CLASSES).  Classes:
  far            far away from everything
  inside         inside the first instance's mesh, around the middle of its root box, small: touches nothing when that mesh is closed and hollow
  face           straddling the face of a triangle, at a random orientation
  edge           straddling an edge or a vertex of a triangle
  object         containing one whole instance (its world box, inflated), axis aligned
  scene          containing the whole scene
  thin           slabs (one half extent tiny) and needles (two), through a triangle
  zero_off       zero-extent boxes (points, segments, rectangles) near a surface; the point kind lies OFF it by a clear offset
  rot45_1        turned by 45 degrees about one coordinate axis, straddling a face
  rot45_3        turned by 45 degrees about x, then y, then z
  unnormalised   face boxes whose quaternion is scaled by 1e-3 or 37
  zero_on        a point ON a surface: a triangle's first vertex (exactly, where the instance is unmoved)
  touch_face / touch_corner / touch_edge   exact touching, made only for a scene whose first instance is the unmoved golden `cube` (the
                 mesh [-1, 1]^3): a box face coplanar with the cube's face x = 1, a box corner on the vertex (1, 1, 1) (both exact in fp32), a
                 box edge crossing the cube's edge x = y = 1 at right angles (exact up to the rounding of sqrt(2))
  dead           NaN, inf, a negative half extent, a zero quaternion
NON_TOUCHING names the classes whose offsets from every surface are clear by construction (random, or at least 1e-2 of the local size): the
classes a test may demand equality with the exhaustive search on.  sat_gaps() is the fp64 separating-axis test the header's MARGIN is
checked against."""
import numpy as np

import hitset

f32 = np.float32
CLASSES = ("far", "inside", "face", "edge", "object", "scene", "thin", "zero_off", "rot45_1", "rot45_3", "unnormalised", "zero_on",
           "touch_face", "touch_corner", "touch_edge", "dead")
NON_TOUCHING = ("far", "inside", "face", "edge", "object", "scene", "thin", "zero_off", "rot45_1", "rot45_3", "unnormalised")
IDENTITY = (0.0, 0.0, 0.0, 1.0)
S45 = float(np.sin(np.pi / 8)), float(np.cos(np.pi / 8))          # the half angle of a 45 degree turn


def quat_mul(a, b):
    """a * b for (x, y, z, w) quaternions: b's turn first, then a's."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)


def quat_axes(q):
    """The box axes of a quaternion as rows (3, 3), fp64, normalised first: the columns of Transform::calc_world_matrix's rotation."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    m = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return m.T


def _random_quat(rng):
    q = rng.normal(size=4)
    return tuple(q / np.linalg.norm(q))


def _world_triangle(sc, rng):
    """A random triangle's three world-space vertices (fp64) and whether its instance is unmoved."""
    inst, p0, e1, e2 = hitset._triangle(sc, rng)
    v = np.stack([p0, p0 + e1, p0 + e2])
    m = np.asarray(inst["world"], np.float64).reshape(4, 4)
    unmoved = np.array_equal(m, np.eye(4))
    return (v if unmoved else hitset._xform(inst["world"], v)), unmoved


def is_dead(boxes):
    b = np.asarray(boxes, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        qq = (b[:, 6:].astype(f32) ** 2).sum(axis=1, dtype=f32)
    return ~(np.isfinite(b).all(axis=1) & (b[:, 3:6] >= 0).all(axis=1) & np.isfinite(qq) & (qq > 0))


def generate(sc, n=12, seed=0):
    rng = np.random.default_rng(seed)
    rows, labels = [], []

    def add(name, c, h, q=IDENTITY):
        rows.append(np.concatenate([np.asarray(c, np.float64), np.asarray(h, np.float64), np.asarray(q, np.float64)])); labels.append(CLASSES.index(name))

    lo, hi = hitset.world_box(sc)
    ext = hi - lo
    has_tris = len(sc.tlas_nodes) > 0 and len(sc.instances) > 0
    for k in range(n):
        add("far", hi + ext * (2.0 + rng.uniform(0, 1, 3)) * np.where(rng.uniform(size=3) < 0.5, -1.0, 1.0) - np.where(k % 2, ext * 6, 0), rng.uniform(0.05, 0.5, 3) * ext.min(), _random_quat(rng))
        add("scene", 0.5 * (lo + hi) + rng.uniform(-0.1, 0.1, 3) * ext, ext * rng.uniform(1.5, 2.5), _random_quat(rng) if k % 2 else IDENTITY)
    if has_tris:
        inst0 = sc.instances[0]
        root = sc.blas[int(inst0["blas_id"])].nodes[0]
        rlo, rhi = root["aabb_min"].astype(np.float64), root["aabb_max"].astype(np.float64)
        for k in range(n):
            # inside: around the middle of the first mesh's root box, in its own frame, turned with the instance
            c_l = 0.5 * (rlo + rhi) + rng.uniform(-0.15, 0.15, 3) * (rhi - rlo)
            add("inside", hitset._xform(inst0["world"], c_l), rng.uniform(0.02, 0.12, 3) * (rhi - rlo).min(), _random_quat(rng))
            # object: one instance's world box, inflated
            leaf = sc.instances[int(rng.integers(len(sc.instances)))]
            r = sc.blas[int(leaf["blas_id"])].nodes[0]
            corners = np.array([[(r["aabb_max"] if (j >> a) & 1 else r["aabb_min"])[a] for a in range(3)] for j in range(8)], np.float64)
            w = hitset._xform(leaf["world"], corners)
            add("object", 0.5 * (w.min(axis=0) + w.max(axis=0)), 0.5 * (w.max(axis=0) - w.min(axis=0)) * rng.uniform(1.1, 1.4) + 0.05)
            # face, edge, thin, zero_off, rot45, unnormalised, zero_on: at a random triangle
            v, unmoved = _world_triangle(sc, rng)
            size = max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[0]), 1e-3)
            nrm = np.cross(v[1] - v[0], v[2] - v[0]); nl = np.linalg.norm(nrm)
            nrm = nrm / nl if nl > 0 else np.array([0.0, 0.0, 1.0])
            bary = rng.dirichlet((2, 2, 2))
            on_face = bary @ v
            add("face", on_face + nrm * rng.uniform(-0.05, 0.05) * size, rng.uniform(0.1, 0.4, 3) * size, _random_quat(rng))
            e = int(rng.integers(3)); t = rng.uniform(0, 1) if k % 2 else 0.0
            on_edge = v[e] * (1 - t) + v[(e + 1) % 3] * t
            add("edge", on_edge + rng.uniform(-0.03, 0.03, 3) * size, rng.uniform(0.08, 0.3, 3) * size, _random_quat(rng))
            thin = rng.uniform(0.5, 1.5, 3) * size
            thin[rng.permutation(3)[:1 + k % 2]] = 1e-3 * size
            add("thin", on_face + nrm * rng.uniform(-0.02, 0.02) * size, thin, _random_quat(rng))
            z = rng.uniform(0.1, 0.5, 3) * size
            z[[a for a in range(3) if ((1 + k % 7) >> a) & 1]] = 0.0
            add("zero_off", on_face + nrm * (0.05 + rng.uniform(0, 0.2)) * size * (1 if k % 4 < 2 else -1) * (1.0 if not z.any() else rng.uniform(0, 1)), z, _random_quat(rng))
            a1 = [0.0, 0.0, 0.0, S45[1]]; a1[k % 3] = S45[0]
            add("rot45_1", on_face + nrm * rng.uniform(-0.04, 0.04) * size, rng.uniform(0.1, 0.4, 3) * size, tuple(a1))
            qx, qy, qz = (S45[0], 0, 0, S45[1]), (0, S45[0], 0, S45[1]), (0, 0, S45[0], S45[1])
            add("rot45_3", on_face + nrm * rng.uniform(-0.04, 0.04) * size, rng.uniform(0.1, 0.4, 3) * size, quat_mul(qz, quat_mul(qy, qx)))
            add("unnormalised", on_face + nrm * rng.uniform(-0.05, 0.05) * size, rng.uniform(0.1, 0.4, 3) * size, tuple(np.array(_random_quat(rng)) * (1e-3 if k % 2 else 37.0)))
            add("zero_on", v[0], (0.0, 0.0, 0.0), _random_quat(rng) if k % 2 else IDENTITY)
        m0 = np.asarray(inst0["world"], np.float64).reshape(4, 4)
        if np.array_equal(m0, np.eye(4)) and np.array_equal(rlo, [-1, -1, -1]) and len(sc.blas[int(inst0["blas_id"])].tri_hot) == 12:
            for k in range(n):                                           # face and corner: every number is exact in fp32, and so is every sum the test forms
                hx, hy, hz = 0.25 * (1 + k % 3), 0.5, 0.125 * (1 + k % 5)
                add("touch_face", (1.0 + hx, 0.25 * (k % 4) - 0.5, 0.125 * (k % 7) - 0.25), (hx, hy, hz))
                add("touch_corner", (1.0 + hx, 1.0 + hy, 1.0 + hz), (hx, hy, hz))
                # turned 45 degrees about x: the box's lowest edge runs along x at height y = 1 and crosses the cube's edge x = 1, y = 1 (and the
                # face's diagonal) at right angles — touching up to the rounding of sqrt(2), the one class here that is not exact
                add("touch_edge", (1.0, 1.0 + np.sqrt(2.0) * hz, 0.25 * (k % 5) - 0.5), (0.5, hz, hz), (S45[0], 0.0, 0.0, S45[1]))
    for k in range(n):
        c, h, q = rng.uniform(-1, 1, 3), rng.uniform(0.1, 1, 3), np.array(_random_quat(rng))
        kind = k % 6
        if kind == 0: c[k % 3] = np.nan
        elif kind == 1: h[k % 3] = np.inf
        elif kind == 2: h[k % 3] = -0.125
        elif kind == 3: q[:] = 0.0
        elif kind == 4: q[k % 4] = np.nan
        else: c[k % 3] = -np.inf
        add("dead", c, h, q)
    with np.errstate(over="ignore"):
        return np.array(rows).astype(f32), np.array(labels)


def in_classes(labels, names):
    return np.isin(labels, [CLASSES.index(c) for c in names])


def sat_gaps(row, inst, hot):
    """The fp64 separating-axis test of one live box row against every triangle of one instance: (gaps (T, 13), kappas (T, 13), S (T,), W).
    gaps: the signed distance between the projections of box and triangle on each NORMALISED axis (3 box axes, the normal, 9 cross axes),
    positive when separated, -inf for an axis of zero length (it never separates); kappas: the conditioning of each axis as MARGIN defines it;
    S = |d0| + |e1| + |e2| + |h|; W = |c| + |c_l|, 0 for an identity matrix."""
    r = np.asarray(row, np.float64)
    c, h = r[:3], r[3:6]
    A = quat_axes(r[6:10])
    M = np.asarray(inst["world_inv"], np.float64).reshape(4, 4)
    c_l = M[:3, :3] @ c + M[:3, 3]
    A = A @ M[:3, :3].T                                                   # rows: the local axes
    W = 0.0 if np.array_equal(M, np.eye(4)) else float(np.linalg.norm(c) + np.linalg.norm(c_l))
    p0, e1, e2 = (np.asarray(hot[k], np.float64) for k in ("position_0", "position_edge_1", "position_edge_2"))
    v0, f1, f2 = (p0 - c_l) @ A.T, e1 @ A.T, e2 @ A.T
    V = np.stack([v0, v0 + f1, v0 + f2], axis=1)                          # (T, 3 vertices, 3)
    T = len(p0)
    gaps = np.full((T, 13), -np.inf); kappas = np.ones((T, 13))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(3):
            gaps[:, k] = np.maximum(V[:, :, k].min(axis=1) - h[k], -V[:, :, k].max(axis=1) - h[k])

        def axis(col, a, cond_num):
            la = np.linalg.norm(a, axis=1)
            p = np.einsum("tvk,tk->tv", V, a)
            rad = np.abs(a) @ h
            ok = la > 0
            g = np.maximum(p.min(axis=1) - rad, -p.max(axis=1) - rad)
            gaps[ok, col] = g[ok] / la[ok]
            kappas[ok, col] = cond_num[ok] / la[ok]
        axis(3, np.cross(f1, f2), np.linalg.norm(f1, axis=1) * np.linalg.norm(f2, axis=1))
        col = 4
        for f in (f1, f2 - f1, f2):
            for i in range(3):
                e = np.zeros(3); e[i] = 1.0
                axis(col, np.cross(np.broadcast_to(e, f.shape), f), np.linalg.norm(f, axis=1)); col += 1
    S = np.linalg.norm(p0 - c_l, axis=1) + np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1) + np.linalg.norm(h)
    return gaps, kappas, S, W
