"""Object masks and row masks for the filtered walk queries (Renderer.query_nearest / query_hits / query_sweep with mask=..., the host twins
with mask= and object_masks=), like pointset.py for points:
  object_masks     seeded random masks over 4 bits (0 .. 15: an object with mask 0 exists for nobody), one per object in the numbering of the
                   object_id channel (instances, spheres, planes); hide_world: the spheres and the planes get 0
  coincident_masks the golden scene "coincident": its instances, two of which are the same mesh in the same place, get one bit each
  row_masks        per-row masks drawn from {0, one bit, two bits, all ones}, with rows of mask 0 planted on both sides of every wave boundary
  visible_scene    the scene with the hidden objects REALLY removed (a balanced TLAS over the instances left) and the map back to its ids
The rule: an object exists for a row iff (object mask & row mask) != 0."""
import copy

import numpy as np

f32 = np.float32
u32 = np.uint32
ALL_ONES = 0xFFFFFFFF
BITS = 4
WAVE = 64


def object_count(sc):
    return len(sc.instances) + len(sc.spheres) + len(sc.planes)


def object_masks(sc, seed, hide_world=False):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << BITS, object_count(sc)).astype(u32)
    if hide_world:
        m[len(sc.instances):] = 0
    return m


def coincident_masks(sc):
    """One bit per instance (instances 0 and 1 coincide), every bit for the rest."""
    ni = len(sc.instances)
    assert ni <= BITS and np.array_equal(sc.instances[0]["world"], sc.instances[1]["world"]) and sc.instances[0]["blas_id"] == sc.instances[1]["blas_id"]
    m = np.full(object_count(sc), (1 << BITS) - 1, u32)
    m[:ni] = 1 << np.arange(ni)
    return m


def row_masks(n, seed):
    """(n,) uint32 from {0, one bit, two bits, all ones}; rows 63, 64, 127, 128, ... (below n) hold 0."""
    rng = np.random.default_rng(seed)
    one = [1 << b for b in range(BITS)]
    two = [a | b for i, a in enumerate(one) for b in one[i + 1:]]
    kind = rng.integers(0, 8, n)                                   # 1/8 zero, 3/8 one bit, 2/8 two bits, 2/8 all ones
    m = np.where(kind == 0, 0, np.where(kind < 4, rng.choice(one, n), np.where(kind < 6, rng.choice(two, n), ALL_ONES))).astype(u32)
    for w in range(WAVE, n, WAVE):
        m[w - 1] = 0
        m[w] = 0
    return m


def visible(table, object_ids, row_masks_):
    """Per element of object_ids (any shape; rows along axis 0): the object exists for the element's row.  -1 (no object) -> True."""
    ids = np.asarray(object_ids)
    rm = np.asarray(row_masks_, u32).reshape((-1,) + (1,) * (ids.ndim - 1))
    t = np.asarray(table, u32)
    return (ids < 0) | ((t[np.clip(ids, 0, len(t) - 1)] & rm) != 0)


def _world_boxes(sc, keep):
    """World boxes of instances `keep`, (k, 6) float32, rounded outwards: every corner of the mesh's root box through the instance matrix."""
    out = np.zeros((len(keep), 6), f32)
    for j, i in enumerate(keep):
        b = sc.blas[int(sc.instances[i]["blas_id"])].nodes[0]
        lo, hi = b["aabb_min"].astype(np.float64), b["aabb_max"].astype(np.float64)
        corners = np.array([[hi[0] if k & 1 else lo[0], hi[1] if k & 2 else lo[1], hi[2] if k & 4 else lo[2]] for k in range(8)])
        m = sc.instances[i]["world"].astype(np.float64).reshape(4, 4)
        w = corners @ m[:3, :3].T + m[:3, 3]
        pad = 1e-5 * (1.0 + np.abs(w).max())
        out[j, :3] = np.nextafter((w.min(axis=0) - pad).astype(f32), f32(-np.inf))
        out[j, 3:] = np.nextafter((w.max(axis=0) + pad).astype(f32), f32(np.inf))
    return out


def visible_scene(sc, table, row_mask):
    """(scene without the objects hidden from row_mask, ids): ids[k] = the object id in `sc` of object k of the new scene.  The TLAS is
    host.tlas_build_balanced over the instances left; None when no instance, sphere or plane is left."""
    from pyrtx import host
    table = np.asarray(table, u32)
    ni, ns = len(sc.instances), len(sc.spheres)
    vis = (table & u32(row_mask & ALL_ONES)) != 0
    ki, ks, kp = np.flatnonzero(vis[:ni]), np.flatnonzero(vis[ni:ni + ns]), np.flatnonzero(vis[ni + ns:])
    if len(ki) + len(ks) + len(kp) == 0:
        return None, np.zeros(0, np.int64)
    out = copy.copy(sc)
    out.instances = sc.instances[ki].copy()
    out.spheres = sc.spheres[ks].copy()
    out.planes = sc.planes[kp].copy()
    if len(ki):
        boxes = _world_boxes(sc, ki)
        out.tlas_nodes, out.tlas_indices = host.tlas_build_balanced((boxes[:, :3] + boxes[:, 3:]) * f32(0.5), boxes)
    else:
        out.tlas_nodes, out.tlas_indices = sc.tlas_nodes[:0].copy(), np.zeros(0, np.int32)
    return out, np.concatenate([ki, ni + ks, ni + ns + kp])
