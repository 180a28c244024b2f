"""rtxh_blas_build_balanced, the host twin of rtx_alloc_blas + rtx_build_blas (csrc/rtx_build_math.h compiled for the CPU): the specification
the device arrays are compared with in tests/test_gpu_blas_build.py.  Everything is compared bit for bit; nothing here is a tolerance.

  properties   for thirteen triangle counts, on random soups, all-identical triangles and hostile vertices: node count and depth are the two
               shape functions, leaf ranges lie inside the arrays, the slot table is a permutation, every reachable box is finite, ordered and
               nested, both wide walks' upload conditions hold (build_nodes_pk4 / pk4c's rules restated), invalid triangles occupy the lowest
               slots with NaN hot records and widen no box;
  refit        rtxh_blas_refit on the twin's own output with the same vertices returns the same boxes;
  frames       the oracle renders Torus and Monkey with the balanced tree; the count of pixels that differ from the frame of the SBVH tree
               of the same mesh is recorded, and equality is asserted where that count is 0.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import util
from test_blas_refit_cpu import build, hostile_vertices, load_soup, reachable, tori_scene

f32 = np.float32
LEAF_MAX = 4
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 1000, 70000]
NAN_BITS = 0x7fc00000
INT32_MIN = -2 ** 31


def soup(n, seed=0, kind="random"):
    """-> positions (3n, 3), indices (n, 3), normals (3n, 3), texcoords (3n, 2), material ids (n,)"""
    rng = np.random.default_rng(1000 * seed + n)
    c = rng.uniform(-4, 4, (n, 1, 3))
    pos = (c + rng.normal(0, 0.15, (n, 3, 3))).astype(f32).reshape(-1, 3)
    if kind == "identical":
        pos = np.tile(np.array([[1.5, -2.0, 0.25], [2.5, -2.0, 0.25], [1.5, -1.0, 0.75]], f32), (n, 1))
    elif kind == "hostile":
        m = rng.random(pos.shape)
        pos[m < 0.05] = np.nan; pos[(m > 0.1) & (m < 0.15)] = np.inf; pos[(m > 0.2) & (m < 0.25)] = -np.inf
        pos[(m > 0.3) & (m < 0.33)] = f32(3e38); pos[(m > 0.4) & (m < 0.43)] = f32(-3e38); pos[(m > 0.5) & (m < 0.52)] = f32(1e-41)
    idx = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    nrm = rng.normal(0, 1, (3 * n, 3)).astype(f32)
    uv = rng.uniform(0, 1, (3 * n, 2)).astype(f32)
    mid = rng.integers(0, 3, n).astype(np.int32)
    return pos, idx, nrm, uv, mid


def with_invalid(idx, V, seed=3):
    """Every fifth triangle gets a bad index, the four kinds in turn -> (indices, the invalid source triangles)."""
    idx = idx.copy()
    bad = list(range(0, len(idx), 5))
    for j, t in enumerate(bad):
        if j % 4 == 0: idx[t] = -1
        elif j % 4 == 1: idx[t, 2] = V
        elif j % 4 == 2: idx[t, 0] = INT32_MIN
        else: idx[t, 1] = -1; idx[t, 2] = V + 7
    return idx, np.array(bad)


def levels_of(n):
    L = 0
    while -(-n // (1 << L)) > LEAF_MAX:
        L += 1
    return L


def wide_conditions(nodes, tri_count):
    """build_nodes_pk4 / build_nodes_pk4c of csrc/rtx_layout_host.h restated: min <= max, leaves below 16 triangles, even `left`, children nested in
    the stored floats, fewer than 2^24 nodes and triangles.  -> (pk4 need with smallest need first, pk4c need)"""
    n = len(nodes)
    assert n < (1 << 24) and tri_count < (1 << 24)
    mn, mx = nodes["aabb_min"], nodes["aabb_max"]
    cnt = nodes["count"] & 0x3fffffff
    left = nodes["left_or_first"]
    order = reachable(nodes)
    need4, need4c = {}, {}
    for i in order:
        assert (mn[i] <= mx[i]).all()
        if cnt[i] > 0:
            assert cnt[i] < 16
            continue
        l = int(left[i])
        assert l % 2 == 0
        for c in (l, l + 1):
            assert (mn[c] >= mn[i]).all() and (mx[c] <= mx[i]).all(), (i, c)
    for i in reversed(order):                                       # pre-order reversed: children before parents
        if cnt[i] > 0:
            need4[i] = need4c[i] = 0
            continue
        l = int(left[i])
        slots = []
        for c in (l, l + 1):
            slots += [c] if cnt[c] > 0 else [int(left[c]), int(left[c]) + 1]
        ns = len(slots)
        by_need = sorted(need4[s] for s in slots)
        need4[i] = max((ns - 1 - t) + v for t, v in enumerate(by_need))
        need4c[i] = max(need4c[s] for s in slots) + ns - 1
    return need4[0], need4c[0]


def check_tree(blas, sv, order, pos, idx, expect_invalid=()):
    """The invariants of the twin's output, whatever the input.  Returns the reachable node indices."""
    from pyrtx import host
    n = len(idx); V = len(pos)
    nodes = blas.nodes
    L = levels_of(n)
    assert len(nodes) == host.blas_balanced_node_count(n) == 2 << L
    assert host.blas_balanced_inner_depth(n) == L - 1
    reach = reachable(nodes)
    r = np.array(reach)
    mn, mx = nodes["aabb_min"], nodes["aabb_max"]
    assert np.isfinite(mn[r]).all() and np.isfinite(mx[r]).all() and (mn[r] <= mx[r]).all()
    unreach = np.setdiff1d(np.arange(len(nodes)), r)
    assert not nodes[unreach].tobytes().strip(b"\0"), "holes and index 1 are zero bytes"
    assert sorted(order.tolist()) == list(range(n)), "the slot table is a permutation of the source triangles"
    # depth of every inner node and the leaf ranges: the heap of rtx_build_math.h
    covered = np.zeros(n, np.int32)
    depth = {0: 0}
    deepest_inner = -1
    for i in reach:
        cnt, f = int(nodes["count"][i]) & 0x3fffffff, int(nodes["left_or_first"][i])
        d = depth[i]
        j = i - (1 << d) if d else 0
        first, end = (j * n) >> d, ((j + 1) * n) >> d
        if cnt == 0:
            assert end - first > LEAF_MAX and f == (2 << d) | (2 * j) and f + 1 < len(nodes)
            assert 1 <= (int(nodes["count"][i]) >> 30) & 3 <= 3, "an inner node carries an axis"
            depth[f] = depth[f + 1] = d + 1
            deepest_inner = max(deepest_inner, d)
        else:
            assert (first, end - first) == (f, cnt) and cnt <= LEAF_MAX and 0 <= f and f + cnt <= n
            assert int(nodes["count"][i]) >> 30 == 0
            covered[f:f + cnt] += 1
    assert (covered == 1).all(), "every slot lies in exactly one leaf"
    assert deepest_inner == L - 1
    # validity
    valid_src = ((idx >= 0) & (idx < V)).all(1)
    assert np.array_equal(np.flatnonzero(~valid_src), np.asarray(expect_invalid, np.int64).reshape(-1))
    valid = valid_src[order]
    # the key's top bit: valid AND a finite box (every axis has a finite component); triangles without it occupy the lowest slots in index order
    tri = pos[np.where(valid_src[:, None], idx, 0)]
    bit = (valid_src & np.isfinite(tri).any(1).all(1))[order]
    k_inv = int((~bit).sum())
    assert not bit[:k_inv].any() and bit[k_inv:].all(), "invalid triangles (and those without a finite box) occupy the lowest slots"
    assert np.array_equal(order[:k_inv], np.sort(order[:k_inv])), "in index order"
    assert (sv[~valid] == -1).all() and np.array_equal(sv[valid], idx[order][valid])
    hot = blas.tri_hot
    raw = np.frombuffer(hot.tobytes(), np.uint32).reshape(n, 9)
    assert (raw[~valid] == NAN_BITS).all(), "nine constant quiet NaNs"
    cold0 = blas.tri_cold[~valid]
    for fld in ("tex_coord_0", "tex_coord_edge_1", "tex_coord_edge_2", "normal_0", "normal_edge_1", "normal_edge_2"):
        assert not cold0[fld].tobytes().strip(b"\0")
    p = pos[np.where(valid[:, None], sv, 0)]                       # (n, 3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    v = valid
    assert util.bit_exact(hot["position_0"][v], p[v, 0]) and util.bit_exact(hot["position_edge_1"][v], e1[v]) and util.bit_exact(hot["position_edge_2"][v], e2[v])
    # every finite vertex component of a valid triangle inside its leaf's box; an invalid triangle widens no box: the leaf's box is the
    # box of its valid triangles alone (refit rule: min / max over the finite components, [+0, +0] on an axis without one, then the fix)
    for i in reach:
        cnt, f = int(nodes["count"][i]) & 0x3fffffff, int(nodes["left_or_first"][i])
        if cnt == 0:
            continue
        q = p[f:f + cnt][valid[f:f + cnt]].reshape(-1, 3)
        for a in range(3):
            col = q[:, a][np.isfinite(q[:, a])] if len(q) else q[:, a]
            lo, hi = (f32(col.min()), f32(col.max())) if len(col) else (f32(0), f32(0))
            assert mn[i][a] == lo and float(hi) <= float(mx[i][a]) <= float(hi) + 0.0101, (i, a)      # fix_if_needed raises max by 0.005, per triangle and per leaf
    return reach


def twin(pos, idx, nrm, uv=None, mid=None):
    from pyrtx import host
    return host.blas_build_balanced(pos, idx, nrm, uv, mid)


def refit_of_twin(blas, sv, pos, nrm=None):
    """rtxh_blas_refit on the twin's output; invalid slots are emulated by an appended NaN vertex (and an appended zero normal: the cold
    record of an invalid triangle stays zero)."""
    from pyrtx import host
    V = len(pos)
    sv2 = np.where(sv < 0, V, sv).astype(np.int32)
    pos2 = np.concatenate([pos, np.full((1, 3), np.nan, f32)])
    nrm2 = None if nrm is None else np.concatenate([nrm, np.zeros((1, 3), f32)])
    return host.blas_refit(blas, sv2, pos2, nrm2)


@pytest.mark.parametrize("kind", ["random", "identical", "hostile"])
@pytest.mark.parametrize("n", COUNTS)
def test_properties_of_the_twin(n, kind):
    pos, idx, nrm, uv, mid = soup(n, 1, kind)
    blas, sv, order = twin(pos, idx, nrm, uv, mid)
    check_tree(blas, sv, order, pos, idx)
    need4, need4c = wide_conditions(blas.nodes, n)
    assert need4 <= 36 and need4c <= 62, "RTX_PK4_MAX_NEED, RTX_MAX_STACK - 2: the mesh takes both 4-wide walks"
    if kind == "identical":
        assert np.array_equal(order, np.arange(n)), "ties are broken by the source index (every centre falls into cell 0 / 0)"
    # the cold records: host.build_blas's arithmetic on the gathered vertices
    c = blas.tri_cold
    assert np.array_equal(c["material_id"], mid[order])
    assert util.bit_exact(c["normal_0"], nrm[sv[:, 0]]) and util.bit_exact(c["normal_edge_2"], nrm[sv[:, 2]] - nrm[sv[:, 0]])
    assert util.bit_exact(c["tex_coord_0"], uv[sv[:, 0]]) and util.bit_exact(c["tex_coord_edge_1"], uv[sv[:, 1]] - uv[sv[:, 0]])
    no_uv, _, _ = twin(pos, idx, nrm, None, None)
    assert not no_uv.tri_cold["tex_coord_edge_2"].tobytes().strip(b"\0") and (no_uv.tri_cold["material_id"] == 0).all()
    assert no_uv.nodes.tobytes() == blas.nodes.tobytes() and no_uv.tri_hot.tobytes() == blas.tri_hot.tobytes()
    # consistency with the refit
    again = refit_of_twin(blas, sv, pos, nrm)
    assert again.nodes.tobytes() == blas.nodes.tobytes()
    assert util.bit_exact(again.tri_hot["position_edge_1"], blas.tri_hot["position_edge_1"]) and again.tri_cold.tobytes() == blas.tri_cold.tobytes()


@pytest.mark.parametrize("kind", ["random", "hostile"])
@pytest.mark.parametrize("n", COUNTS)
def test_invalid_triangles_sort_first_and_widen_no_box(n, kind):
    pos, idx, nrm, uv, mid = soup(n, 2, kind)
    bad_idx, bad = with_invalid(idx, len(pos))
    blas, sv, order = twin(pos, bad_idx, nrm, uv, mid)
    check_tree(blas, sv, order, pos, bad_idx, expect_invalid=bad)
    wide_conditions(blas.nodes, n)
    assert np.array_equal(blas.tri_cold["material_id"], mid[order]), "an invalid triangle keeps its material id"
    again = refit_of_twin(blas, sv, pos, nrm)
    assert again.nodes.tobytes() == blas.nodes.tobytes() and again.tri_cold.tobytes() == blas.tri_cold.tobytes()
    # vertices nobody may read: the indices of invalid triangles point nowhere, the result does not depend on the rest of such a triangle
    other = bad_idx.copy(); other[bad] = -1
    b2, sv2, order2 = twin(pos, other, nrm, uv, mid)
    assert b2.nodes.tobytes() == blas.nodes.tobytes() and np.array_equal(order2, order) and np.array_equal(sv2, sv)


def test_morton_order_keeps_neighbours_together():
    """Not a tolerance on quality, a sanity check of the sort key: on a uniform cloud the leaves of the balanced tree are far smaller than
    the leaves over the unsorted order would be."""
    pos, idx, nrm, _, _ = soup(1000, 5)
    blas, sv, order = twin(pos, idx, nrm)
    leaves = [i for i in reachable(blas.nodes) if int(blas.nodes["count"][i]) & 0x3fffffff]
    ext = np.array([(blas.nodes["aabb_max"][i] - blas.nodes["aabb_min"][i]).max() for i in leaves])
    assert np.median(ext) < 2.0, np.median(ext)                    # the cloud spans 8 units; four random triangles span about 5


def mesh_as_indexed(mesh):
    pos, nrm, uv, mid = load_soup(mesh)
    n = len(pos)
    return pos.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(n, 3), nrm.reshape(-1, 3), uv.reshape(-1, 2), mid


# pixels of the oracle's 16-instance frame that differ between the balanced tree and the SBVH tree of the same mesh, measured on the CPU
# when this test was written; hits do not depend on the tree except at exact ties and ulp-level box edges
FRAME_DIFF = {"Torus": 0, "Monkey": 0}


@pytest.mark.parametrize("mesh", ["Torus", "Monkey"])
def test_oracle_frame_with_the_balanced_tree(mesh):
    import orc
    pos, idx, nrm, uv, mid = mesh_as_indexed(mesh)
    blas, sv, order = twin(pos, idx, nrm, uv, mid)
    check_tree(blas, sv, order, pos, idx)
    ref_blas = build(mesh, reference_sbvh=True)[0]
    a = orc.OracleScene(tori_scene(blas)).render(threads=8)
    b = orc.OracleScene(tori_scene(ref_blas)).render(threads=8)
    diff = int((a["packed"] != b["packed"]).sum())
    print(f"{mesh}: {diff} pixels differ between the balanced tree and the SBVH tree")
    assert diff == FRAME_DIFF[mesh]
    if diff == 0:
        assert a["stats"] == b["stats"] and util.bit_exact(a["rgb"], b["rgb"])


def test_hostile_vertices_hide_only_their_own_triangles():
    import orc
    pos, idx, nrm, uv, mid = mesh_as_indexed("Torus")
    soup_pos, _, _, _ = load_soup("Torus")
    verts, bad = hostile_vertices(soup_pos)
    blas, sv, order = twin(verts, idx, nrm, uv, mid)
    check_tree(blas, sv, order, verts, idx)
    keep = np.setdiff1d(np.arange(len(idx)), bad)
    fresh, _, _ = twin(pos, idx[keep], nrm, uv, mid[keep])
    a = orc.OracleScene(tori_scene(blas)).render(threads=8)
    b = orc.OracleScene(tori_scene(fresh)).render(threads=8)
    assert a["stats"] == b["stats"] and util.bit_exact(a["rgb"], b["rgb"]) and np.array_equal(a["packed"], b["packed"])


def test_argument_checks_and_abi():
    from pyrtx import api, host
    L = host.lib()
    one = np.zeros(64, np.int32)
    nc = C.c_int32()
    p = one.ctypes.data
    assert L.rtxh_blas_build_balanced(p, p, p, None, None, 0, 3, p, C.byref(nc), p, p, p, p) == 1
    assert L.rtxh_blas_build_balanced(p, p, p, None, None, 1, 0, p, C.byref(nc), p, p, p, p) == 1
    assert L.rtxh_blas_build_balanced(None, p, p, None, None, 1, 3, p, C.byref(nc), p, p, p, p) == 1
    neg = np.array([-1], np.int32)
    assert L.rtxh_blas_build_balanced(p, p, p, None, neg.ctypes.data, 1, 3, p, C.byref(nc), p, p, p, p) == 1
    assert L.rtxh_blas_build_balanced(p, p, p, None, None, 1 << 24, 3, p, C.byref(nc), p, p, p, p) == 4
    assert host.blas_balanced_node_count(0) == 0 and host.blas_balanced_node_count(1 << 24) == 0
    assert [host.blas_balanced_node_count(n) for n in (1, 4, 5, 8, 9, 16, 17)] == [2, 2, 4, 4, 8, 8, 16]
    assert [host.blas_balanced_inner_depth(n) for n in (1, 4, 5, 8, 9, (1 << 24) - 1)] == [-1, -1, 0, 0, 1, 21]
    with pytest.raises(ValueError):
        host.blas_build_balanced(np.zeros((3, 3), f32), np.zeros((1, 3), np.int32), np.zeros((2, 3), f32))
    lib = api.load_library()
    for name in api.BUILD_EXPORTS:
        assert hasattr(lib, name) and name in api.EXPORTS, name
    assert lib.rtx_alloc_blas(None, 0, 1, 1, None, 0) == 1 and lib.rtx_build_blas(None, 0, None, None, None, None, None) == 1
