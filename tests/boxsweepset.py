"""Labelled rows for the swept-box queries (rtx_query_sweep_box; csrc/rtx_boxsweep_math.h), seeded, for any scene the query walks.

generate(sc, n, seed) -> (rows float32 (N, 14) of (centre, direction, max distance, half extents, quaternion x y z w), labels int (N,) into
CLASSES).  Classes:
  free           far from everything, flying away: no answer
  approach       a box at a random orientation flying at a triangle's face from its circumscribed distance: mostly a corner onto the face
  face_on        a box with one axis along the triangle's normal, flying along it: a box axis wins (the normal axis ties with it)
  edge_edge      a box edge flying at a triangle's edge at right angles to both: a cross axis wins where the edge is a convex one
  vertex_face    a box face flying at a mesh vertex along the line from the middle of the scene through it
  parallel       hovering over a face and moving along it (vL == 0 on the normal where the numbers are exact)
  overlap        starts overlapping: boxset's face, edge and thin rows with a random direction
  zero1 / zero2 / zero3   approach rows with one, two, three zero half extents (a rectangle, a segment, a point: a ray)
  unnormalised   approach rows whose quaternion is scaled by 1e-3 or 37
  d_inf          approach rows with D = +inf (the others carry a finite D beyond the contact)
  sphere_out / sphere_in / sphere_cross   towards a scene sphere from outside; from inside it towards its shell; starting across the shell
  plane_to / plane_from   towards a scene plane; away from it
  touch          boxset's exact touching rows on the golden cube (t = 0), moving away or along
  graze_hit / graze_miss / d_below / d_above   made by graze_rows() and d_rows(), which need a bound or a contact time: see there
  dead           every dead-row kind: NaN, inf, a zero direction, a negative half extent, a zero quaternion, D <= 0, D NaN
cube_cases() are the analytic rows on the golden cube.  gaps_at() is the fp64 anchor: boxset.sat_gaps with the box moved to c + t d."""
import numpy as np

import boxset
import hitset

f32 = np.float32
CLASSES = ("free", "approach", "face_on", "edge_edge", "vertex_face", "parallel", "overlap", "zero1", "zero2", "zero3", "unnormalised", "d_inf",
           "sphere_out", "sphere_in", "sphere_cross", "plane_to", "plane_from", "touch", "dead", "graze_hit", "graze_miss", "d_below", "d_above")
IDENTITY = boxset.IDENTITY
AXIS_OVERLAP, AXIS_SPHERE, AXIS_PLANE = 13, 14, 15


def row(c, d, D, h, q=IDENTITY):
    return np.concatenate([np.asarray(c, np.float64), np.asarray(d, np.float64), [float(D)], np.asarray(h, np.float64), np.asarray(q, np.float64)]).astype(f32)


def box_of(rows):
    """The (n, 10) rows of query_overlap for the same boxes where they start."""
    r = np.asarray(rows, f32)
    return np.ascontiguousarray(np.concatenate([r[:, 0:3], r[:, 7:14]], axis=1))


def box_at(rows, t):
    """The (n, 10) fp64 boxes moved to c + t d."""
    r = np.asarray(rows, np.float64)
    return np.concatenate([r[:, 0:3] + r[:, 3:6] * np.asarray(t, np.float64)[:, None], r[:, 7:14]], axis=1)


def is_dead(rows):
    r = np.asarray(rows, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        ray = np.isfinite(r[:, :6]).all(axis=1) & (r[:, 3:6] != 0).any(axis=1) & (r[:, 6] > 0)
    return ~ray | boxset.is_dead(box_of(r))


def quat_from_axes(a0, a1):
    """The quaternion (x, y, z, w) whose box axes are a0, a1 (orthonormalised) and a0 x a1."""
    a0 = np.asarray(a0, np.float64); a0 = a0 / np.linalg.norm(a0)
    a1 = np.asarray(a1, np.float64); a1 = a1 - a0 * (a0 @ a1); a1 = a1 / np.linalg.norm(a1)
    m = np.stack([a0, a1, np.cross(a0, a1)], axis=1)                       # columns: the axes
    w = np.sqrt(max(0.0, 1 + m[0, 0] + m[1, 1] + m[2, 2])) / 2
    if w > 1e-3:
        return ((m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w), w)
    x = np.sqrt(max(0.0, 1 + m[0, 0] - m[1, 1] - m[2, 2])) / 2
    if x > 1e-3:
        return (x, (m[0, 1] + m[1, 0]) / (4 * x), (m[0, 2] + m[2, 0]) / (4 * x), (m[2, 1] - m[1, 2]) / (4 * x))
    y = np.sqrt(max(0.0, 1 - m[0, 0] + m[1, 1] - m[2, 2])) / 2
    if y > 1e-3:
        return ((m[0, 1] + m[1, 0]) / (4 * y), y, (m[1, 2] + m[2, 1]) / (4 * y), (m[0, 2] - m[2, 0]) / (4 * y))
    return (0.0, 0.0, 1.0, 0.0)


def _any_perp(v, rng):
    p = np.cross(v, rng.normal(size=3))
    return p / np.linalg.norm(p)


def generate(sc, n=8, seed=0):
    rng = np.random.default_rng(seed)
    rows, labels = [], []

    def add(name, c, d, D, h, q=IDENTITY):
        rows.append(np.concatenate([np.asarray(c, np.float64), np.asarray(d, np.float64), [float(D)], np.asarray(h, np.float64), np.asarray(q, np.float64)]))
        labels.append(CLASSES.index(name))

    lo, hi = hitset.world_box(sc)
    ext = hi - lo
    mid = 0.5 * (lo + hi)
    has_tris = len(sc.tlas_nodes) > 0 and len(sc.instances) > 0
    for k in range(n):
        out = hitset._unit(rng, 1)[0]
        add("free", mid + out * np.linalg.norm(ext) * (2.0 + rng.uniform()), out * rng.uniform(0.5, 2.0), np.inf if k % 2 else 50.0, rng.uniform(0.05, 0.3, 3) * ext.min(), boxset._random_quat(rng))
    if has_tris:
        for k in range(n):
            v, unmoved = boxset._world_triangle(sc, rng)
            size = max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[0]), 1e-3)
            nrm = np.cross(v[1] - v[0], v[2] - v[0]); nl = np.linalg.norm(nrm)
            nrm = nrm / nl if nl > 0 else np.array([0.0, 0.0, 1.0])
            if nrm @ (v.mean(axis=0) - mid) < 0:
                nrm = -nrm                                                  # away from the middle of the scene: mostly the open side
            on_face = rng.dirichlet((2, 2, 2)) @ v
            h = rng.uniform(0.1, 0.4, 3) * size
            reach = np.linalg.norm(h)
            speed = rng.uniform(0.3, 3.0)
            tilt = _any_perp(nrm, rng) * rng.uniform(0, 0.3)
            far = 8.0 * (reach + size)
            add("approach", on_face + nrm * reach * rng.uniform(1.2, 2.5), (-nrm + tilt) * speed, far, h, boxset._random_quat(rng))
            add("d_inf", on_face + nrm * reach * rng.uniform(1.2, 2.5), (-nrm + tilt) * speed, np.inf, h, boxset._random_quat(rng))
            add("unnormalised", on_face + nrm * reach * rng.uniform(1.2, 2.5), -nrm * speed, far, h, tuple(np.array(boxset._random_quat(rng)) * (1e-3 if k % 2 else 37.0)))
            qn = quat_from_axes(nrm, _any_perp(nrm, rng))
            add("face_on", on_face + nrm * (h[0] + size * rng.uniform(0.2, 1.0)), -nrm * speed, far, h, qn)
            # edge against edge: the box edge along a_i through a point off the triangle's edge, both at right angles to the motion
            e = k % 3
            ea, eb = v[e], v[(e + 1) % 3]
            fdir = (eb - ea) / max(np.linalg.norm(eb - ea), 1e-12)
            A = boxset.quat_axes(boxset._random_quat(rng))
            i = (k // 3) % 3
            N = np.cross(A[i], fdir)
            if np.linalg.norm(N) > 1e-3:
                N = N / np.linalg.norm(N)
                if N @ (0.5 * (ea + eb) - v.mean(axis=0)) < 0 or (abs(N @ nrm) > 0.5 and N @ nrm < 0):
                    N = -N
                j, l = (i + 1) % 3, (i + 2) % 3
                corner = -np.sign(N @ A[j]) * h[j] * A[j] - np.sign(N @ A[l]) * h[l] * A[l]
                q_e = quat_from_axes(A[0], A[1])
                add("edge_edge", 0.5 * (ea + eb) + N * size * rng.uniform(0.2, 0.6) - corner + A[i] * rng.uniform(-0.3, 0.3) * h[i], -N * speed, far, h, q_e)
            u = v[k % 3] - mid                                              # away from the middle of the scene: at a convex vertex the vertex meets the face
            u = u / np.linalg.norm(u) if np.linalg.norm(u) > 1e-6 else nrm
            add("vertex_face", v[k % 3] + u * (h[0] + size * rng.uniform(0.2, 0.8)) + _any_perp(u, rng) * 0.3 * min(h[1], h[2]), -u * speed, far, h, quat_from_axes(u, _any_perp(u, rng)))
            add("parallel", on_face + nrm * (h[0] + size * rng.uniform(0.05, 0.3)), _any_perp(nrm, rng) * speed, 4.0 * size, h, qn)
            z = h.copy()
            for kind, name in ((1, "zero1"), (2, "zero2"), (3, "zero3")):
                z = h.copy(); z[rng.permutation(3)[:kind]] = 0.0
                add(name, on_face + nrm * (reach * 1.2 + 0.1 * size), (-nrm + tilt) * speed, far, z, boxset._random_quat(rng))
        boxes, lab = boxset.generate(sc, max(2, n // 2), seed=seed + 1)
        for b in boxes[boxset.in_classes(lab, ("face", "edge", "thin"))]:
            add("overlap", b[:3], hitset._unit(rng, 1)[0] * rng.uniform(0.5, 2.0), 10.0, b[3:6], b[6:10])
        for k, b in enumerate(boxes[boxset.in_classes(lab, ("touch_face", "touch_corner"))]):
            add("touch", b[:3], (1.0, 0.0, 0.0) if k % 2 else (0.0, 1.0, 0.0), 4.0, b[3:6], b[6:10])
    for s in sc.spheres:
        c, R = s["center"].astype(np.float64), float(np.sqrt(s["radius_squared"]))
        for k in range(max(2, n // 2)):
            out = hitset._unit(rng, 1)[0]
            h = rng.uniform(0.05, 0.25, 3) * R
            add("sphere_out", c + out * (R + np.linalg.norm(h) * 1.5 + 0.2 * R), (-out + _any_perp(out, rng) * rng.uniform(0, 0.2)) * rng.uniform(0.5, 2.0), 10.0 * R, h, boxset._random_quat(rng))
            add("sphere_in", c + out * 0.2 * R, hitset._unit(rng, 1)[0] * rng.uniform(0.5, 2.0), 10.0 * R, h * 0.5, boxset._random_quat(rng))
            add("sphere_cross", c + out * R, hitset._unit(rng, 1)[0], 10.0 * R, h, boxset._random_quat(rng))
    for p in sc.planes:
        nv, dist = p["normal"].astype(np.float64), float(p["distance"])
        for k in range(max(2, n // 2)):
            on = -nv * dist + _any_perp(nv, rng) * rng.uniform(0, 3.0)
            side = 1.0 if k % 2 else -1.0
            h = rng.uniform(0.1, 0.5, 3)
            add("plane_to", on + nv * side * (np.linalg.norm(h) + rng.uniform(0.2, 2.0)), (-nv * side + _any_perp(nv, rng) * 0.3) * rng.uniform(0.5, 2.0), 100.0, h, boxset._random_quat(rng))
            add("plane_from", on + nv * side * (np.linalg.norm(h) + rng.uniform(0.2, 2.0)), (nv * side + _any_perp(nv, rng) * 0.3) * rng.uniform(0.5, 2.0), 100.0, h, boxset._random_quat(rng))
    for k in range(2 * n):
        c, d, D, h, q = rng.uniform(-1, 1, 3), hitset._unit(rng, 1)[0], 5.0, rng.uniform(0.1, 1, 3), np.array(boxset._random_quat(rng))
        kind = k % 10
        if kind == 0: c[k % 3] = np.nan
        elif kind == 1: d[k % 3] = np.inf
        elif kind == 2: d[:] = (0.0, -0.0, 0.0)
        elif kind == 3: h[k % 3] = -0.125
        elif kind == 4: q[:] = 0.0
        elif kind == 5: D = 0.0
        elif kind == 6: D = -1.0
        elif kind == 7: D = np.nan
        elif kind == 8: h[k % 3] = np.inf
        else: q[k % 4] = np.nan
        add("dead", c, d, D, h, q)
    with np.errstate(over="ignore"):
        return np.array(rows).astype(f32), np.array(labels)


def in_classes(labels, names):
    return np.isin(labels, [CLASSES.index(c) for c in names])


def d_rows(rows, t):
    """For answered rows with t > 0: the same rows with D just below the contact (no answer) and just above it (the same answer)."""
    r = np.asarray(rows, f32)
    below, above = r.copy(), r.copy()
    below[:, 6] = np.nextafter(np.asarray(t, f32), f32(0)); above[:, 6] = np.nextafter(np.asarray(t, f32), f32(np.inf))
    return below, above


def graze_rows(clearances, h=(0.25, 0.5, 0.375)):
    """Identity boxes flying along +y past the unmoved golden cube's face x = 1 at the given signed clearances (negative: it bites)."""
    return np.stack([row((1.0 + h[0] + g, -3.0, 0.125), (0.0, 1.0, 0.0), 20.0, h) for g in clearances])


S45 = boxset.S45


def cube_cases():
    """Analytic rows against the unmoved golden cube [-1, 1]^3, each (row, t, axis set, normal): every number exact in fp32 unless noted."""
    r2 = np.sqrt(2.0)
    qz = (0.0, 0.0, S45[0], S45[1])                                        # 45 degrees about z: the box's x-y section is a diamond
    qx, qy = (S45[0], 0.0, 0.0, S45[1]), (0.0, S45[0], 0.0, S45[1])
    return [
        (row((3.0, 0.25, -0.125), (-1.0, 0.0, 0.0), 10.0, (0.5, 0.25, 0.125)), 1.5, {0}, (1.0, 0.0, 0.0)),                 # face on: the box axis x (the normal ties)
        (row((3.0, 0.25, -0.125), (-2.0, 0.0, 0.0), 10.0, (0.5, 0.25, 0.125)), 0.75, {0}, (1.0, 0.0, 0.0)),                # t is in units of |d|
        (row((0.25, -4.0, 0.5), (0.0, 0.5, 0.0), np.inf, (0.25, 1.0, 0.25)), 4.0, {1}, (0.0, -1.0, 0.0)),
        (row((3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 10.0, (0.5, 0.5, 0.25), qz), 2.0 - 0.5 * r2, {3}, (1.0, 0.0, 0.0)),          # edge on: the box's vertical edge onto the face
        (row((4.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 10.0, (0.5, 0.5, 0.5), boxset.quat_mul(qz, qy)),
         3.0 - 0.5 * float(np.abs(boxset.quat_axes(boxset.quat_mul(qz, qy))[:, 0]).sum()), {3}, (1.0, 0.0, 0.0)),             # corner on: 45 degrees about y, then about z; the box reaches 0.5 sum |a_k.x| along x
        (row((3.0, 3.0, 0.0), (-1.0, -1.0, 0.0), 10.0, (0.5, 0.5, 0.25)), 1.5, {0, 1}, None),                                 # the box's edge meets the cube's edge x = y = 1 head on: two box axes tie
        (row((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 10.0, (0.25, 0.25, 0.25)), 0.75, {0}, (-1.0, 0.0, 0.0)),                    # inside the hollow cube, towards its face x = 1
        (row((0.0, 0.5, 0.0), (1.0, 0.0, 0.0), 10.0, (0.0, 0.0, 0.0)), 1.0, {0, 3}, (-1.0, 0.0, 0.0)),                     # a point box: a ray
        (row((3.0, 0.0, 0.0), (1.0, 0.0, 0.0), 10.0, (0.5, 0.5, 0.5)), np.inf, {-1}, (0.0, 0.0, 0.0)),                     # flying away
        (row((3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 1.4375, (0.5, 0.5, 0.5)), np.inf, {-1}, (0.0, 0.0, 0.0)),                  # D short of the contact
        (row((1.5, 0.0, 0.0), (-1.0, 0.0, 0.0), 10.0, (0.5, 0.5, 0.5)), 0.0, {AXIS_OVERLAP}, (0.0, 0.0, 0.0)),             # starts touching, exactly
        (row((1.25, 0.0, 0.0), (0.0, 1.0, 0.0), 10.0, (0.5, 0.5, 0.5)), 0.0, {AXIS_OVERLAP}, (0.0, 0.0, 0.0)),             # starts overlapping
    ]


def chain_rows(n=12):
    """Fat boxes flying along -x from beyond the last triangle of test_gpu_rays.chain_blas_scene(): at every step of the chain the rest is the
    nearer child and the leaf is pushed, one stack entry per level (23) before the first triangle is tested."""
    ys = np.linspace(-0.3, 0.3, n)
    return np.stack([row((6.0, ys[k], 0.1), (-1.0, 0.01 * (k % 3 - 1), 0.0), np.inf if k % 2 else 20.0, (0.05, 0.4, 0.4), IDENTITY if k % 3 == 0 else (0.1, 0.2, 0.3, 0.9)) for k in range(n)])


COS_FLOOR = 0.25          # contacts compared in t are those whose normal is within 75.5 degrees of the motion: a distance bound b is b / (|d| cos) in t


def world_scale(sc, p):
    """W of the headers' MARGIN for a world point p: |p| + |p in the instance's frame|, the largest over the instances; 0 where every matrix is the identity."""
    p = np.asarray(p, np.float64)
    w = 0.0
    for inst in sc.instances:
        m = np.asarray(inst["world_inv"], np.float64).reshape(4, 4)
        if not np.array_equal(m, np.eye(4)):
            w = max(w, float(np.linalg.norm(p) + np.linalg.norm(m[:3, :3] @ p + m[:3, 3])))
    return w


def contact(sc, row14, t, obj, slot, normal):
    """Of a triangle answer: (S, W, kappa of the axis with the largest exact gap at t, that axis, cos of the returned normal to the motion,
    whether the bound excludes it: kappa beyond 2^10, or the normal axis of a sliver beyond 4), all fp64."""
    inst = sc.instances[obj]
    hot = sc.blas[int(inst["blas_id"])].tri_hot
    g, kap, S, W = gaps_at(row14, t, inst, hot[slot:slot + 1])
    k = int(np.argmax(g[0]))
    e1, e2 = hot["position_edge_1"][slot].astype(np.float64), hot["position_edge_2"][slot].astype(np.float64)
    nl = np.linalg.norm(np.cross(e1, e2))
    sliver = np.inf if nl == 0 else np.linalg.norm(e1) * np.linalg.norm(e2) / nl
    d = np.asarray(row14[3:6], np.float64)
    cos = abs(float(np.asarray(normal, np.float64) @ d)) / float(np.linalg.norm(d))
    return float(S[0]), float(W), float(kap[0, k]), k, cos, bool(kap[0, k] > 2 ** 10 or (k == 3 and sliver > 4)), float(sliver), float(g[0, k])


def gaps_at(row14, t, inst, hot):
    """boxset.sat_gaps for the box of one row moved to c + t d: (gaps (T, 13), kappas, S, W), all fp64."""
    return boxset.sat_gaps(box_at(np.asarray(row14)[None], np.array([t]))[0], inst, hot)
