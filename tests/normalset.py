"""Shared inputs of the vertex-normal tests (tests/test_vertex_normals_cpu.py, tests/test_gpu_vertex_normals.py): the golden meshes indexed by
their OBJ `v` lines, a numpy float32 restatement of the specification (include/rtx.h, device-side vertex normals) written a third way — per
triangle, vectorised over corners in ascending order — small synthetic shapes, the rule cases and the hostile floats."""
import functools
import os

import numpy as np

import util

f32 = np.float32
MESHES = os.path.join(util.GOLDEN, "meshes")
I32_MIN = -2 ** 31


@functools.lru_cache(maxsize=None)
def _load(mesh):
    verts, vns, faces, face_vn = [], [], [], []
    with open(os.path.join(MESHES, mesh + ".obj")) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                verts.append([float(x) for x in p[1:4]])
            elif p[0] == "vn":
                vns.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                c = [q.split("/") for q in p[1:]]
                for k in range(2, len(c)):                       # a polygon as a fan from its first vertex
                    tri = (c[0], c[k - 1], c[k])
                    faces.append([int(q[0]) - 1 for q in tri])
                    face_vn.append([int(q[2]) - 1 for q in tri])
    return (np.array(verts, f32), np.array(faces, np.int32), np.array(vns, np.float64), np.array(face_vn, np.int64))


def indexed(mesh):
    """-> (positions (V, 3) f32, indices (T, 3) i32): the OBJ's `v` lines and its faces into them."""
    v, f, _, _ = _load(mesh)
    return v.copy(), f.copy()


def corner_vn(mesh):
    """-> (T, 3, 3) float64: the file's own `vn` at every corner."""
    _, _, vn, fvn = _load(mesh)
    return vn[fvn]


def valid_triangles(indices, V):
    i = np.asarray(indices, np.int64).reshape(-1, 3)
    return ((i >= 0) & (i < V)).all(1)


def numpy_normals(positions, indices, subnormal_mask=False):
    """The specification in numpy float32, every operation rounded to fp32 in the order the header states.
    subnormal_mask=True: also a (V,) bool array — a subnormal edge, product, face component or partial sum was met on the way to that vertex."""
    pos = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    V = len(pos)
    tiny = np.finfo(f32).tiny
    sub = lambda x: bool(np.any((x != 0) & (np.abs(x) < tiny)))
    acc = np.zeros((V, 3), f32)
    seen = np.zeros(V, bool)
    with np.errstate(all="ignore"):
        for t in np.nonzero(valid_triangles(idx, V))[0]:
            i0, i1, i2 = idx[t]
            e1 = pos[i1] - pos[i0]; e2 = pos[i2] - pos[i0]
            f = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], f32)
            if not np.isfinite(f).all():
                f = np.zeros(3, f32)
            s = sub(e1) or sub(e2) or sub(np.outer(e1, e2)) or sub(f)
            for k in (i0, i1, i2):
                acc[k] = acc[k] + f
                seen[k] |= s or sub(acc[k])
        out = np.zeros((V, 3), f32)
        m = np.abs(acc).max(1)
        ok = np.isfinite(acc).all(1) & (m > 0)
        a = acc[ok] / m[ok][:, None]
        d = a[:, 0] * a[:, 0] + (a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        out[ok] = a / np.sqrt(d)[:, None]
    return (out, seen) if subnormal_mask else out


def is_zero(normals):
    """(V,) bool: exact +0 +0 +0."""
    return (np.ascontiguousarray(normals, f32).view(np.uint32).reshape(-1, 3) == 0).all(1)


def lengths(normals):
    return np.sqrt((np.asarray(normals, np.float64) ** 2).sum(1))


def neighbours(indices, V, v):
    """The vertices that share a valid triangle with v (v included)."""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    idx = idx[valid_triangles(idx, V)]
    return np.unique(idx[(idx == v).any(1)])


# ---- synthetic shapes: the smallest that cross the kernels' edges (256-lane workgroups over corners, triangles and vertices) -------------
def soup(T, V, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (V, 3)).astype(f32), rng.integers(0, V, (T, 3)).astype(np.int32)


def fan(valence, seed=0):
    """Vertex 0 in the middle of `valence` triangles over a ring: one list of that length."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(valence) / valence
    ring = np.stack([np.cos(a), 0.05 * rng.uniform(-1, 1, valence), np.sin(a)], 1)
    pos = np.concatenate([[[0.0, 0.3, 0.0]], ring]).astype(f32)
    k = np.arange(valence)
    return pos, np.stack([np.zeros(valence, np.int64), 1 + (k + 1) % valence, 1 + k], 1).astype(np.int32)


def grid(rows, cols):
    """A closed grid of rows x cols vertices, two triangles per cell: V = rows * cols, valence 6."""
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    a, b = 2 * np.pi * i / rows, 2 * np.pi * j / cols + 0.3
    pos = np.stack([(2 + 0.7 * np.cos(b)) * np.cos(a), 0.7 * np.sin(b), (2 + 0.7 * np.cos(b)) * np.sin(a)], -1).reshape(-1, 3).astype(f32)
    p = i * cols + j; q = i * cols + (j + 1) % cols; r = ((i + 1) % rows) * cols + j; s = ((i + 1) % rows) * cols + (j + 1) % cols
    return pos, np.stack([np.stack([p, r, q], -1), np.stack([q, r, s], -1)], 2).reshape(-1, 3).astype(np.int32)


def shapes():
    """name -> (positions, indices)"""
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32), np.array([[0, 1, 2]], np.int32))
    point = (np.array([[1, 2, 3]], f32), np.array([[0, 0, 0]], np.int32))
    return {"T1": one, "V1": point, "T85": soup(85, 40, 1), "T86": soup(86, 40, 2), "V255": grid(15, 17), "V256": grid(16, 16),
            "V257": grid(257, 1), "fan65": fan(65, 3), "fan257": fan(257, 4)}


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------
def padded(indices, V):
    """Invalid triangles woven into a mesh: -1 padding, indices >= V and INT32_MIN in one corner each, and whole -1 rows at the end."""
    idx = np.asarray(indices, np.int32).reshape(-1, 3)
    bad = [-1, V, V + 7, I32_MIN, 2 ** 31 - 1]
    rows = []
    for t, tri in enumerate(idx):
        if t % 5 == 0:
            b = tri.copy(); b[(t // 5) % 3] = bad[(t // 5) % 5]
            rows.append(b)
        rows.append(tri)
    rows += [np.full(3, -1, np.int32)] * 2
    return np.array(rows, np.int32)


def rule_cases():
    """name -> (positions, indices, the mesh whose normals it must equal (positions, indices) or None, all normals zero?)"""
    pos, idx = indexed("icosphere")
    V = len(pos)
    twice = np.insert(idx, 30, [4, 4, 9], axis=0)
    unused = np.concatenate([pos, [[5, 5, 5]]]).astype(f32)
    dead = idx.copy()
    dead[np.arange(len(idx)), np.arange(len(idx)) % 3] = np.where(np.arange(len(idx)) % 2, -1, V)
    return {"padded": (pos, padded(idx, V), (pos, idx), False), "vertex_twice": (pos, twice, (pos, idx), False),
            "unused_vertex": (unused, idx, None, False), "all_invalid": (pos, dead, None, True)}


HOSTILE = [(np.nan, np.nan, np.nan), (np.inf, 0.0, 0.0), (0.5, -np.inf, 0.25), (3e38, 3e38, -3e38), (-3e38, 0.1, 0.2),
           (1e-41, -1e-42, 1e-45), (-0.0, -0.0, -0.0), (np.nan, np.inf, -3e38)]


def hostile_cases():
    """-> [(positions, indices, planted vertex)]: icosphere with one hostile vertex each, and one with eight spread over the mesh (vertex -1)."""
    pos, idx = indexed("icosphere")
    out = []
    for h, val in enumerate(HOSTILE):
        p = pos.copy(); v = (11 + 29 * h) % len(pos)
        with np.errstate(over="ignore"):
            p[v] = np.array(val, f32)
        out.append((p, idx, v))
    p = pos.copy()
    for h, val in enumerate(HOSTILE):
        p[(11 + 29 * h) % len(pos)] = np.array(val, f32)
    out.append((p, idx, -1))
    return out
