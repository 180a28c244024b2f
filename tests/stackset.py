"""Scenes in which the TLAS and a mesh are BOTH deep, their cameras, and a numpy replay of the packet kernels' shared closest-hit walk.

A wave of the packet kernels keeps ONE stack of RTX_PK_STACK = 64 entries for the TLAS part and the BLAS part of a walk together
(csrc/rtx_limits.h), where the reference has 64 entries per BVH; plan_stack_limits (csrc/rtx_plan.h) decides on the host which scenes the
packet kernels may take.  two_chains builds the scenes that sit on that rule's bounds: n instances in a row under a chain-shaped TLAS, each
instance the same mesh of m triangles in a row under a chain-shaped BVH, everything along the world x axis so that rays travelling along
the row pass through every leaf box of both trees.

packet_stack_high_water replays pk_walk's readable C++ branch (csrc/rtx_packet.h) for one packet of 64 rays and reports how many stack
entries that walk has pending at most.  It is a tool for choosing inputs and for stating conditions on them; no device value is ever
compared with it.  No GPU is needed by anything in this module.
"""
import collections
import copy

import numpy as np

import util
from pyrtx import api, host, scene_io as sio

PK_STACK = 64            # RTX_PK_STACK, csrc/rtx_limits.h
PK_FIFO = 48             # RTX_PK_FIFO, csrc/rtx_packet.h: a lane turns private only while (sp - floor_sp) + 2 <= RTX_PK_FIFO
RAY_EPSILON = 0.005      # Ray.h:5
SIZE = 32                # frames are one tile
BLOCK = (slice(8, 16), slice(8, 16))      # the packet the cameras are aimed with: the 8x8 pixel block (1, 1) of the tile
TRI_PITCH = 0.02         # triangles of the mesh along local x
GAP = 0.1                # free space between two instances
PX = 0.001               # cameras (a) and (b): tangent of the angle between neighbouring pixels

AXES_CYCLE = "cycle"

Figures = collections.namedtuple("Figures", "dt blas_any blas_shared tlas_inner_depth blas_inner_depth")
HighWater = collections.namedtuple("HighWater", "sp rel few_rel steps")


def _chain(boxes, rest_left, axes, pair_leaf=False):
    """Reference-style node array (root 0, node 1 unused, children in pairs) of a chain over items 0 .. k-1 with the leaf boxes `boxes`
    (k, 6): the inner node of level d holds the leaf of item d and the rest of the chain, the rest as the left or the right child.
    pair_leaf: the last two items share the deepest leaf (first = k - 2, count 2), so the chain is one level shorter."""
    if pair_leaf:
        assert len(boxes) >= 3
        merged = np.concatenate([boxes[:-2], np.concatenate([boxes[-2:, :3].min(axis=0), boxes[-2:, 3:].max(axis=0)])[None, :]])
        nodes = _chain(merged, rest_left, axes)
        last = [j for j in range(len(nodes)) if j != 1 and (int(nodes[j]["count"]) & 0x3fffffff) == 1 and int(nodes[j]["left_or_first"]) == len(merged) - 1][0]
        nodes[last]["count"] = 2
        return nodes
    k = len(boxes)
    nodes = np.zeros(max(2 * k, 1), sio.BVH_NODE)
    if k == 1:
        nodes = nodes[:1]
        nodes[0]["aabb_min"] = boxes[0, :3]; nodes[0]["aabb_max"] = boxes[0, 3:]; nodes[0]["left_or_first"] = 0; nodes[0]["count"] = 1
        return nodes
    at = 0                                                           # index of the inner node of level d
    for d in range(k - 1):
        axis = (1 + d % 3) if axes == AXES_CYCLE else int(axes)
        nodes[at]["aabb_min"] = boxes[d:, :3].min(axis=0); nodes[at]["aabb_max"] = boxes[d:, 3:].max(axis=0)
        nodes[at]["left_or_first"] = 2 * d + 2; nodes[at]["count"] = np.uint32(axis << 30).astype(np.int32)
        rest, leaf = (2 * d + 2, 2 * d + 3) if rest_left else (2 * d + 3, 2 * d + 2)
        nodes[leaf]["aabb_min"] = boxes[d, :3]; nodes[leaf]["aabb_max"] = boxes[d, 3:]; nodes[leaf]["left_or_first"] = d; nodes[leaf]["count"] = 1
        at = rest
    nodes[at]["aabb_min"] = boxes[k - 1, :3]; nodes[at]["aabb_max"] = boxes[k - 1, 3:]; nodes[at]["left_or_first"] = k - 1; nodes[at]["count"] = 1
    return nodes


def mesh_length(m):
    return TRI_PITCH * m


def row_positions(n, m):
    """World x of the centres of the n instances."""
    return (mesh_length(m) + GAP) * np.arange(n, dtype=np.float64)


# instance k of n is rotated about the row's axis (quaternions x, y, z, w): a quarter turn swaps the local y and z directions and flips one
# sign, the eighth turn mixes them, so that the lanes of one packet disagree differently in those instances than in world space
ROT_QUARTER = (0.70710678, 0.0, 0.0, 0.70710678)
ROT_EIGHTH = (0.38268343, 0.0, 0.0, 0.92387953)


def rotation_of(k, n):
    if n >= 2 and k == n - 1: return ROT_EIGHTH      # the bottom of the TLAS chain, entered with the most TLAS entries pending
    if n >= 3 and k == 1: return ROT_QUARTER
    return (0.0, 0.0, 0.0, 1.0)


def two_chains(n, m, tlas_rest_left=True, blas_rest_left=True, axes=AXES_CYCLE, bounces=2, pair_leaf=False):
    """n instances of one mesh of m triangles, both trees chains (inner depths n - 2 and m - 2); cube's materials (made reflective) and
    light plus a point light on the row's axis beyond its far end, whose shadow rays run along the row.  The last instance — the bottom of
    the TLAS chain — is the one turned by an eighth: lanes that agree on the signs of d.y and d.z in world space disagree on one of them
    in its model space.  pair_leaf: the last two instances share the deepest TLAS leaf (inner depth n - 3): the iterator entry of that leaf
    lies below the BLAS part of the first of them."""
    assert n >= 1 and m >= 2
    sc, _ = util.load_golden("cube")
    sc = copy.deepcopy(sc)
    hot = np.zeros(m, sio.TRI_HOT); cold = np.zeros(m, sio.TRI_COLD)
    # slivers along a diagonal of their leaf box that passes the row's axis at 0.04 to 0.13: every leaf box spans y >= -0.5 and |z| <= 0.3
    # around the axis, while rays near the axis thread through many triangles before one stops them, each at its own depth
    for i in range(m):
        s = 1.0 if i % 2 == 0 else -1.0
        x = TRI_PITCH * (i - 0.5 * (m - 1)) - 0.0075
        hot["position_0"][i] = (x, -0.5, -0.3 * s); hot["position_edge_1"][i] = (0.015, 1.1 + 0.1 * (i % 3), 0.6 * s); hot["position_edge_2"][i] = (0.005, 0.04, 0.0)
        nrm = np.array([-1.0, 0.3 * ((i % 5) - 2), 0.2 * ((i % 7) - 3)])      # a normal of its own per triangle: a hit on the wrong one is another colour
        cold["normal_0"][i] = nrm / np.linalg.norm(nrm); cold["material_id"][i] = sc.blas[0].tri_cold["material_id"][0]
    p = np.stack([hot["position_0"], hot["position_0"] + hot["position_edge_1"], hot["position_0"] + hot["position_edge_2"]]).astype(np.float32)
    tri_boxes = np.concatenate([p.min(axis=0), p.max(axis=0)], axis=1)
    sc.blas = [sio.Blas(_chain(tri_boxes, blas_rest_left, axes), hot, cold, sc.blas[0].material_offset, m)]
    root = sc.blas[0].nodes[0]
    inst = np.zeros(n, sio.INSTANCE); boxes = np.zeros((n, 6), np.float32)
    for k, x in enumerate(row_positions(n, m)):
        one, mn, mx = host.instance_update((x, 0.0, 0.0), rotation_of(k, n), root["aabb_min"], root["aabb_max"], 0)
        inst[k] = one[0]; boxes[k, :3] = mn; boxes[k, 3:] = mx
    sc.instances, sc.tlas_nodes, sc.tlas_indices = inst, _chain(boxes, tlas_rest_left, axes, pair_leaf), np.arange(n, dtype=np.int32)
    sc.materials["reflection"][:] = 0.4
    end = float(row_positions(n, m)[-1]) + 0.5 * mesh_length(m)
    pl = np.zeros(len(sc.point_lights) + 1, sio.POINT_LIGHT)
    pl[0]["colour"] = (6.0, 5.0, 4.0); pl[0]["position"] = (end + 2.0, 0.021, -0.017)      # first light: on the axis, beyond the far end
    pl[1:] = sc.point_lights
    sc.point_lights = pl
    sc.spheres = sc.spheres[:0]; sc.planes = sc.planes[:0]
    sc.config["width"] = SIZE; sc.config["height"] = SIZE; sc.config["bounces"] = bounces; sc.config["stack_size"] = 64; sc.config["traversal_strategy"] = 1
    sc.camera = camera_along(n, m, +1)
    return sc


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
def camera_along(n, m, direction):
    """(a) direction +1 / (b) direction -1: a pinhole camera on the row's axis outside one end, looking along it.  The ray of zero
    transverse direction lies between pixels 11 and 12 in both image directions, so the lanes of block (1, 1) disagree on the signs of
    d.y and d.z; the whole block stays within 0.2 of the axis over the longest row of the grid."""
    xs = row_positions(n, m)
    lo, hi = xs[0] - 0.5 * mesh_length(m), xs[-1] + 0.5 * mesh_length(m)
    cam = np.zeros(1, sio.CAMERA)
    cam["position"] = ((lo - 1.5) if direction > 0 else (hi + 1.5), 0.013, -0.009)
    cam["rotated_x_axis"] = (0.0, 0.0, PX * direction); cam["rotated_y_axis"] = (0.0, -PX, 0.0)
    cam["rotated_top_left_corner"] = (float(direction), 11.5 * PX, -11.5 * PX * direction)
    return cam


def _parallel_rays(targets_yz, x_at, direction3):
    """(32, 32, 18) rays of one direction through the points (x_at, y, z) of targets_yz (32, 32, 2), origins 3 units before them."""
    d = np.asarray(direction3, np.float64); d = d / np.linalg.norm(d)
    rays = np.zeros((SIZE, SIZE, api.RAY_FLOATS), np.float32)
    t = np.zeros((SIZE, SIZE, 3)); t[..., 0] = x_at; t[..., 1:] = targets_yz
    rays[..., 0:3] = t - 3.0 * d; rays[..., 3:6] = d
    return rays


def rays_parallel(n, m, sign=+1):
    """(c) an orthographic block: parallel rays (every lane has the same direction signs: no sign split parks anything) through a 0.02
    grid around the axis at the last instance."""
    j, i = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    yz = np.stack([-(j - 11.5) * 0.02 + 0.004, (i - 11.5) * 0.02 + 0.003], axis=-1)
    return _parallel_rays(yz, float(row_positions(n, m)[-1]), (sign * 1.0, sign * 0.002, sign * 0.003))


def rays_silhouette(sc, sign=+1):
    """(d) rays parallel in the model space of the LAST instance of which, in block (1, 1), only lanes (i, j) = (8, 8) and (9, 8) pass the
    boxes of that instance: the others run below its y = -0.5 or beyond its z = 0.3, the two planes every leaf box of the mesh shares.
    sign: the sign of all three model-space direction components (+1 makes a chain whose rest is the left child the near child at every
    node, -1 one whose rest is the right child)."""
    j, i = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing="ij")
    w = sc.instances[len(sc.instances) - 1]["world"].astype(np.float64).reshape(4, 4)
    local = np.zeros((SIZE, SIZE, 3)); local[..., 1] = -0.495 - 0.01 * (j - 8); local[..., 2] = 0.285 + 0.01 * (i - 8)
    d = np.array([sign * 1.0, sign * 0.001, sign * 0.0015]); d = w[:3, :3] @ (d / np.linalg.norm(d))
    rays = np.zeros((SIZE, SIZE, api.RAY_FLOATS), np.float32)
    rays[..., 0:3] = local @ w[:3, :3].T + w[:3, 3] - 3.0 * d; rays[..., 3:6] = d
    return rays


def block_rays(rays):
    """The 64 rays (origin, direction) of block (1, 1) of a (32, 32, >= 6) ray view."""
    return np.asarray(rays)[BLOCK][..., :6].reshape(64, 6).astype(np.float64)


def camera_block_rays(cam):
    return block_rays(api.pinhole_rays(cam, SIZE, SIZE))


# ---- the figures the host rule reads -------------------------------------------------------------------------------------------------
def inner_depth(nodes):
    """Depth of the deepest inner node (root = 0), -1 for a tree that is one leaf: tree_inner_depth of the C ABI."""
    best, stack = -1, [(0, 0)]
    while stack:
        i, d = stack.pop()
        if (int(nodes[i]["count"]) & 0x3fffffff) > 0: continue
        best = max(best, d)
        f = int(nodes[i]["left_or_first"])
        stack += [(f, d + 1), (f + 1, d + 1)]
    return best


def figures(sc, pk4_need=None):
    """stack_figures of csrc/rtx_api.hip from the scene's arrays: dt = TLAS levels, blas_any = the deepest mesh's need in the shadow-ray
    walk (pk4_need where the context reports 4-wide records, read back on a GPU; else inner depth + 2 of the binary walk), blas_shared."""
    t = inner_depth(sc.tlas_nodes) if len(sc.tlas_nodes) else -1
    b = max(inner_depth(x.nodes) for x in sc.blas)
    return Figures(t + 1 if len(sc.tlas_nodes) else 0, pk4_need if pk4_need is not None and pk4_need >= 0 else b + 2, 2 * (b + 2), t, b)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
def _slab(lo, hi, o, inv, tcur):
    with np.errstate(invalid="ignore"):
        t0 = (lo - o) * inv; t1 = (hi - o) * inv
    near = np.maximum(RAY_EPSILON, np.minimum(t0, t1).max(axis=1))
    far = np.minimum(tcur, np.maximum(t0, t1).min(axis=1))
    return near < far


def packet_stack_high_water(sc, rays64, ordered=True):
    """pk_walk<ANY = false> of csrc/rtx_packet.h, its readable C++ branch, for one packet: the TLAS descend with sign split, the iterator
    entry of a leaf with more than one instance, entering an instance, the BLAS descend with sign split, the far child pushed with the
    lanes that pass now, the pop-time re-test against each lane's closest distance, the triangle test updating that distance.  No lane
    ever turns private (no hand-over), slab and triangle tests in fp64.  Returns HighWater: sp = the most entries on the stack, rel = the
    most entries of one instance (sp - floor_sp), few_rel = the largest sp - floor_sp at which a BLAS node was wanted by 1 .. 4 lanes
    (-1: never), steps = nodes expanded."""
    r = np.asarray(rays64, np.float64).reshape(64, 6)
    wo, wd = r[:, :3], r[:, 3:6]
    tcur = np.full(64, np.inf)
    tl = sc.tlas_nodes
    T = {"lo": tl["aabb_min"].astype(np.float64), "hi": tl["aabb_max"].astype(np.float64), "first": tl["left_or_first"].astype(np.int64), "count": tl["count"].astype(np.int64) & 0xffffffff}
    B = []
    for b in sc.blas:
        nd = b.nodes
        B.append({"lo": nd["aabb_min"].astype(np.float64), "hi": nd["aabb_max"].astype(np.float64), "first": nd["left_or_first"].astype(np.int64), "count": nd["count"].astype(np.int64) & 0xffffffff,
                  "p0": b.tri_hot["position_0"].astype(np.float64), "e1": b.tri_hot["position_edge_1"].astype(np.float64), "e2": b.tri_hot["position_edge_2"].astype(np.float64)})
    stack = []                       # entries (a, b, mask, idx, iter, pretested)
    hw = {"sp": 0, "rel": 0, "few": -1, "steps": 0}
    floor_sp = -1
    N = T; o, d = wo, wd
    with np.errstate(divide="ignore"):
        inv = 1.0 / d

    def push(a, b, mask, idx, it=False, pre=False):
        stack.append((a, b, mask, idx, it, pre))
        hw["sp"] = max(hw["sp"], len(stack))
        if floor_sp >= 0: hw["rel"] = max(hw["rel"], len(stack) - floor_sp)

    # the packet starts at the TLAS root with the lanes that pass its box
    m = _slab(T["lo"][0], T["hi"][0], o, inv, tcur)
    cur_idx, cur_first, cur_cnt = 0, int(T["first"][0]), int(T["count"][0])
    mesh = None
    while True:
        if m.any():
            if floor_sp >= 0 and 1 <= int(m.sum()) <= 4: hw["few"] = max(hw["few"], len(stack) - floor_sp)
            leafc = cur_cnt & 0x3fffffff
            if leafc > 0:
                if floor_sp >= 0:
                    for i in range(cur_first, cur_first + leafc):
                        p0, e1, e2 = mesh["p0"][i], mesh["e1"][i], mesh["e2"][i]
                        hh = np.cross(d, e2); a = hh @ e1
                        with np.errstate(divide="ignore", invalid="ignore"):
                            f = 1.0 / a
                            s = o - p0; u = f * np.einsum("ij,ij->i", s, hh)
                            q = np.cross(s, e1); v = f * np.einsum("ij,ij->i", d, q); t = f * (q @ e2)
                            hit = (u > 0) & (u < 1) & (v > 0) & (u + v < 1) & (t > RAY_EPSILON) & (t < tcur) & m
                        tcur = np.where(hit, t, tcur)
                else:
                    push(cur_first, leafc, m.copy(), 0, it=True)
                m = np.zeros(64, bool)
            else:
                hw["steps"] += 1
                left_first = True
                axis = cur_cnt >> 30
                if ordered and axis != 0:
                    pos = (d[:, axis - 1] > 0.0) & m
                    if not pos.any(): left_first = False
                    elif (pos != m).any():
                        push(cur_first, cur_cnt, m & ~pos, cur_idx, pre=True)      # the right-first lanes wait on this node
                        m = pos
                left = cur_first
                ml = _slab(N["lo"][left], N["hi"][left], o, inv, tcur) & m
                mr = _slab(N["lo"][left + 1], N["hi"][left + 1], o, inv, tcur) & m
                near, far = (left, left + 1) if left_first else (left + 1, left)
                m_near, m_far = (ml, mr) if left_first else (mr, ml)
                if m_near.any():
                    if m_far.any(): push(int(N["first"][far]), int(N["count"][far]), m_far, far)
                    cur_idx, cur_first, cur_cnt, m = near, int(N["first"][near]), int(N["count"][near]), m_near
                elif m_far.any():
                    cur_idx, cur_first, cur_cnt, m = far, int(N["first"][far]), int(N["count"][far]), m_far
                else:
                    m = np.zeros(64, bool)
            continue
        # pop
        if floor_sp >= 0 and len(stack) == floor_sp:
            if not stack: break
            floor_sp = -1; N = T; o, d = wo, wd
            with np.errstate(divide="ignore"):
                inv = 1.0 / d
        if not stack: break
        ea, eb, em, eidx, it, pre = stack.pop()
        if it:
            if eb > 1: push(ea + 1, eb - 1, em, 0, it=True)
            I = sc.instances[int(sc.tlas_indices[ea])]
            w = I["world_inv"].astype(np.float64).reshape(4, 4)
            o = wo @ w[:3, :3].T + w[:3, 3]; d = wd @ w[:3, :3].T
            with np.errstate(divide="ignore"):
                inv = 1.0 / d
            mesh = B[int(I["blas_id"])]; N = mesh
            floor_sp = len(stack)
            m = _slab(N["lo"][0], N["hi"][0], o, inv, tcur) & em
            cur_idx, cur_first, cur_cnt = 0, int(N["first"][0]), int(N["count"][0])
        else:
            m = em if pre else (_slab(N["lo"][eidx], N["hi"][eidx], o, inv, tcur) & em)
            cur_idx, cur_first, cur_cnt = eidx, ea, eb
    return HighWater(hw["sp"], hw["rel"], hw["few"], hw["steps"])


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
GridScene = collections.namedtuple("GridScene", "name c n m split rest_left axes")
GRID_C = (58, 61, 63, 64, 65, 66)


def grid():
    """c = dt + 1 + blas_any of the binary walk = n + m at 58, 61, 63, 64, 65, 66, each TLAS-heavy (n = 31), balanced (n = c / 2 - 8) and
    mesh-heavy (n = 8; 9 at c = 66 so that m stays at 57), each with the rest of both chains on the left and on the right, split axes
    cycling x, y, z; four more at c = 64 with one constant split axis: 40 scenes of at most 31 instances x 57 triangles."""
    out = []
    for c in GRID_C:
        for split, n in (("tlas", 31), ("even", c // 2 - 8), ("mesh", 8 if c - 8 <= 57 else c - 57)):
            for rest_left in (True, False):
                out.append(GridScene(f"c{c}-{split}-{'L' if rest_left else 'R'}", c, n, c - n, split, rest_left, AXES_CYCLE))
    for axis, rest_left in ((1, True), (2, True), (3, False), (2, False)):
        out.append(GridScene(f"c64-tlas-{'L' if rest_left else 'R'}-axis{axis}", 64, 31, 33, "tlas", rest_left, axis))
    return out


def bound_scenes():
    """c = 59 in the same three splits and on both sides: shared_walk_bound is exactly 64 there, so these are the deepest two chains the
    host rule leaves to the packet kernels (the grid's scenes from c = 61 on take the per-lane kernels)."""
    return [GridScene(f"c59-{split}-{'L' if rest_left else 'R'}", 59, n, 59 - n, split, rest_left, AXES_CYCLE)
            for split, n in (("tlas", 31), ("even", 21), ("mesh", 8)) for rest_left in (True, False)]


def all_scenes():
    return grid() + bound_scenes()


def by_name(name):
    return [g for g in all_scenes() if g.name == name][0]


_scenes = {}


def scene_of(g):
    """The scene of a grid entry, built once per process and never changed by a test."""
    if g.name not in _scenes:
        _scenes[g.name] = two_chains(g.n, g.m, g.rest_left, g.rest_left, g.axes)
    return _scenes[g.name]


def deep_sign(g):
    """The direction sign with which a ray goes to the REST of both chains first at every node: the deep order."""
    return +1 if g.rest_left else -1


def shared_walk_bound(n, m, pair_leaf=False):
    """plan_shared_walk_need (csrc/rtx_plan.h) for a chain TLAS of n instances over a chain mesh of m triangles: one far sibling per
    inner ancestor of a deepest leaf (dt = n - 1 in the TLAS, one fewer where the last two instances share a leaf; m - 1 in the mesh), at
    most three parked entries per tree, and the iterator entry, which the host counts whatever the leaves hold.  Beyond PK_STACK the call
    takes the per-lane kernels."""
    ts, bs = max(n - (2 if pair_leaf else 1), 0), max(m - 1, 0)
    return ts + min(ts, 3) + 1 + bs + min(bs, 3)


# The deepest TLAS leaf holds two instances: 31 instances under a chain of dt = 29 levels.  Over 29 triangles the bound is 64 (packets), over
# 30 it is 65 (per-lane kernels); the iterator entry is really on the stack while the first instance of the pair is walked.
PAIR_LEAF = {"pair-29": (31, 29), "pair-30": (31, 30)}
_pair_scenes = {}


def pair_leaf_scene(name):
    if name not in _pair_scenes:
        n, m = PAIR_LEAF[name]
        _pair_scenes[name] = two_chains(n, m, True, True, AXES_CYCLE, pair_leaf=True)
    return _pair_scenes[name]


_marks = {}


def marks(g):
    """The model's high-water marks of block (1, 1) under the four cameras, computed once per process: {"a", "b", "c", "d"} -> HighWater.
    (c) and (d) use the direction sign that takes the rest of both chains first."""
    if g.name not in _marks:
        sc = scene_of(g)
        _marks[g.name] = {"a": packet_stack_high_water(sc, camera_block_rays(camera_along(g.n, g.m, +1))),
                          "b": packet_stack_high_water(sc, camera_block_rays(camera_along(g.n, g.m, -1))),
                          "c": packet_stack_high_water(sc, block_rays(rays_parallel(g.n, g.m, deep_sign(g)))),
                          "d": packet_stack_high_water(sc, block_rays(rays_silhouette(sc, deep_sign(g))))}
    return _marks[g.name]


FIFO_SCENES = ("c58-mesh-L", "c59-mesh-L", "c59-mesh-R")      # three scenes of the packet kernels whose camera (d) passes the work-list bound (tests/test_packet_stack_cpu.py)


def scene_with_camera(g, which):
    """The grid scene seen by camera "a" or "b" (a shallow copy: the arrays are shared and never written)."""
    sc = copy.copy(scene_of(g))
    sc.camera = camera_along(g.n, g.m, +1 if which == "a" else -1)
    return sc


_frames = {}


def oracle_frame(g, which="a"):
    """The oracle's frame of a grid scene under camera "a" or "b", rendered once per process."""
    import orc
    if (g.name, which) not in _frames:
        _frames[(g.name, which)] = orc.OracleScene(scene_with_camera(g, which)).render(threads=8)
    return _frames[(g.name, which)]
