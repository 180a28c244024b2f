"""rtxh_blas_refit, the host twin of rtx_refit_blas (csrc/rtx_refit_math.h compiled for the CPU): the specification the device arrays are
compared with in tests/test_gpu_blas_refit.py.  Everything is compared bit for bit; nothing here is a tolerance.

  structure   seeded deformations of three meshes (one tree per builder, the SBVH one with duplicated references): every vertex inside its
              leaf's box, children nested, min <= max, topology words and unreachable slots untouched, hot / cold records = host.build_blas's
              arithmetic on the deformed soup gathered by `order`;
  identity    a refit of a reference_bvh tree with the undeformed vertices gives the reference builder's own boxes back;
  frames      the oracle on the refitted tree == the oracle on a tree freshly built on the deformed mesh;
  hostile     NaN, +-inf, all-equal and denormal vertices: the invariants hold, and the frame equals the frame of the mesh without the
              affected triangles.
"""
import copy
import os

import numpy as np
import pytest

import util
from test_tlas_balanced_cpu import poses

f32 = np.float32
MESHES = os.path.join(util.GOLDEN, "meshes")
# mesh, builder arguments of host.build_blas
TREES = {"torus_binned": ("Torus", {}), "icosphere_ref_bvh": ("icosphere", {"reference_bvh": True}), "monkey_ref_sbvh": ("Monkey", {"reference_sbvh": True})}
DEFORMATIONS = ("twist", "wave", "noise", "collapse")


def load_soup(mesh):
    from pyrtx import host
    pos, nrm, uv, mid, _, _ = host.load_obj(os.path.join(MESHES, mesh + ".obj"))
    return pos, nrm, uv, mid


def build(mesh, **kw):
    from pyrtx import host
    pos, nrm, uv, mid = load_soup(mesh)
    return host.build_blas(pos, nrm, uv, mid, 0, **kw), pos, nrm, uv, mid


def deform(verts, kind, seed, amp=1.0):
    """(V, 3) float32 -> (V, 3) float32, seeded; amp scales the displacement (in units of the mesh's extent)."""
    rng = np.random.default_rng(seed)
    v = verts.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max())
    if kind == "twist":                        # rotation about y growing with height
        a = amp * 1.5 * (v[:, 1] - lo[1]) / max(hi[1] - lo[1], 1e-9) + rng.uniform(0, 1)
        c, s = np.cos(a), np.sin(a)
        v = np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], 1)
    elif kind == "wave":
        ph = rng.uniform(0, 6.28)
        v[:, 1] += amp * 0.15 * ext * np.sin(v[:, 0] * (6.0 / ext) + ph) * np.cos(v[:, 2] * (4.0 / ext))
    elif kind == "noise":
        v += rng.normal(0, amp * 0.02 * ext, v.shape)
    elif kind == "collapse":                   # onto the plane y = const: flat boxes everywhere, fix_if_needed at work
        v[:, 1] = lo[1] + 0.25 * (hi[1] - lo[1])
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(v, f32)


def reachable(nodes):
    out, stack = [], [0]
    while stack:
        i = stack.pop(); out.append(i)
        if (int(nodes["count"][i]) & 0x3fffffff) == 0:
            l = int(nodes["left_or_first"][i]); stack += [l, l + 1]
    return out


def check_refit(before, after, sv, verts, normals=None, soup_order=None):
    """The invariants of a refitted BLAS, whatever the vertices.  Returns the reachable node indices."""
    nb, na = before.nodes, after.nodes
    assert na["left_or_first"].tobytes() == nb["left_or_first"].tobytes() and na["count"].tobytes() == nb["count"].tobytes()
    reach = reachable(na)
    unreach = np.setdiff1d(np.arange(len(na)), reach)
    assert na[unreach].tobytes() == nb[unreach].tobytes(), "unreachable slots keep their bytes"
    mn, mx = na["aabb_min"], na["aabb_max"]
    r = np.array(reach)
    assert np.isfinite(mn[r]).all() and np.isfinite(mx[r]).all() and (mn[r] <= mx[r]).all()
    p = verts[sv]                              # (m, 3, 3)
    for i in reach:
        cnt, f = int(na["count"][i]) & 0x3fffffff, int(na["left_or_first"][i])
        if cnt == 0:
            for c in (f, f + 1):
                assert (mn[c] >= mn[i]).all() and (mx[c] <= mx[i]).all(), (i, c)
        else:
            q = p[f:f + cnt].reshape(-1, 3)
            fin = np.isfinite(q)
            assert ((q >= mn[i]) | ~fin).all() and ((q <= mx[i]) | ~fin).all(), i
    # the records: host.build_blas's arithmetic on the deformed soup gathered by `order` (the soup case), else on the gathered vertices
    if soup_order is not None:
        assert np.array_equal(verts.reshape(-1, 3, 3)[soup_order].view(np.uint32), p.view(np.uint32))
    h = after.tri_hot
    with np.errstate(invalid="ignore", over="ignore"):             # inf - inf in the hostile sets
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    assert util.bit_exact(h["position_0"], p[:, 0]) and util.bit_exact(h["position_edge_1"], e1) and util.bit_exact(h["position_edge_2"], e2)
    c0, c1 = before.tri_cold, after.tri_cold
    for fld in ("tex_coord_0", "tex_coord_edge_1", "tex_coord_edge_2", "material_id"):
        assert c1[fld].tobytes() == c0[fld].tobytes(), fld
    if normals is None:
        assert c1.tobytes() == c0.tobytes()
    else:
        n = normals[sv]
        assert util.bit_exact(c1["normal_0"], n[:, 0]) and util.bit_exact(c1["normal_edge_1"], n[:, 1] - n[:, 0]) and util.bit_exact(c1["normal_edge_2"], n[:, 2] - n[:, 0])
    return reach


@pytest.mark.parametrize("kind", DEFORMATIONS)
@pytest.mark.parametrize("tree", list(TREES))
def test_structure_of_refitted_trees(tree, kind):
    from pyrtx import host
    mesh, kw = TREES[tree]
    blas, pos, nrm, uv, mid = build(mesh, **kw)
    if tree == "monkey_ref_sbvh":
        assert len(blas.tri_hot) > len(pos), "the SBVH tree is meant to hold duplicated references"
    sv = host.slot_vertices(blas)
    verts = deform(pos.reshape(-1, 3), kind, seed=7)
    normals = deform(nrm.reshape(-1, 3), "noise", seed=8)
    for nr in (None, normals):
        out = host.blas_refit(blas, sv, verts, nr)
        check_refit(blas, out, sv, verts, nr, soup_order=blas.order)
        fresh = host.build_blas(verts.reshape(-1, 3, 3), (nrm if nr is None else nr).reshape(-1, 3, 3), uv, mid, 0)        # any builder: the records depend on the slot's triangle alone
        src = {int(t): k for k, t in enumerate(fresh.order)}
        k = np.array([src[int(t)] for t in blas.order])
        assert util.bit_exact(out.tri_hot["position_edge_1"], fresh.tri_hot["position_edge_1"][k]) and util.bit_exact(out.tri_cold["normal_edge_2"], fresh.tri_cold["normal_edge_2"][k])


def test_indexed_mesh_through_faces():
    """The same refit through an index buffer: vertices merged by position, faces (n, 3) into them."""
    from pyrtx import host
    blas, pos, *_ = build("Monkey", reference_sbvh=True)
    uniq, inv = np.unique(pos.reshape(-1, 3), axis=0, return_inverse=True)
    faces = inv.reshape(-1, 3).astype(np.int32)
    assert len(uniq) < pos.size // 3 // 2
    sv = host.slot_vertices(blas, faces)
    assert sv.shape == (len(blas.tri_hot), 3) and np.array_equal(uniq[sv].view(np.uint32), pos[blas.order].view(np.uint32))
    verts = deform(np.ascontiguousarray(uniq, f32), "wave", seed=3)
    out = host.blas_refit(blas, sv, verts)
    check_refit(blas, out, sv, verts)
    soup = host.blas_refit(blas, host.slot_vertices(blas), verts[faces].reshape(-1, 3))
    assert out.nodes.tobytes() == soup.nodes.tobytes() and out.tri_hot.tobytes() == soup.tri_hot.tobytes()


@pytest.mark.parametrize("mesh", ["Torus", "icosphere", "Monkey", "Rock", "Cube", "Concave", "Diamond"])
def test_identity_refit_returns_the_reference_builders_boxes(mesh):
    """Identity pin: the box rule (union of the stored child boxes, then fix_if_needed) applied to the undeformed vertices gives every
    reachable node of a reference_bvh tree the box the reference's builder gave it, bit for bit, on all seven meshes:
    BVHPartitions::calculate_bounds unions the boxes of all triangles under a node — a min / max over the same set of floats in another
    order — and no fix fires above the triangles (a fixed triangle box is at least 0.005 wide).  (An SBVH tree is no such pin: a spatial
    split clips child boxes at the split plane, which a refit cannot know.)"""
    from pyrtx import host
    blas, pos, *_ = build(mesh, reference_bvh=True)
    sv = host.slot_vertices(blas)
    out = host.blas_refit(blas, sv, pos.reshape(-1, 3))
    r = np.array(check_refit(blas, out, sv, pos.reshape(-1, 3), soup_order=blas.order))
    assert out.tri_hot.tobytes() == blas.tri_hot.tobytes()
    assert out.nodes[r].tobytes() == blas.nodes[r].tobytes()


def tori_scene(blas, frame=1):
    """tori16 (16 instances of one mesh, three bounces) around the given BLAS: world boxes and balanced TLAS over ITS root box."""
    from pyrtx import host
    sc, _ = util.load_golden("tori16")
    sc = copy.copy(sc)
    sc.blas = [blas]
    pos, rot = poses("tori16", frame)
    sc.instances, sc.tlas_nodes, sc.tlas_indices = host.scene_update_balanced(sc, pos, rot)
    return sc


# (deformation, seed, amplitude) of the torus for the frame comparisons, here and on the GPU
FRAME_CASES = [("twist", 1, 1.0), ("wave", 2, 1.0), ("noise", 3, 0.5)]


def torus_case(kind, seed, amp):
    from pyrtx import host
    blas, pos, nrm, uv, mid = build("Torus", reference_sbvh=True)
    verts = deform(pos.reshape(-1, 3), kind, seed, amp)
    return blas, host.slot_vertices(blas), verts, (nrm, uv, mid)


@pytest.mark.parametrize("kind,seed,amp", FRAME_CASES)
def test_oracle_frame_of_refitted_tree_equals_fresh_build(kind, seed, amp):
    """Hits do not depend on the tree except at exact ties and ulp-level box edges, so the cases are picked: 3 candidates were tried
    (the three listed, the first seed and amplitude written down for each deformation), all 3 gave 0 differing pixels on the oracle."""
    import orc
    from pyrtx import host
    blas, sv, verts, (nrm, uv, mid) = torus_case(kind, seed, amp)
    refit = host.blas_refit(blas, sv, verts)
    fresh = host.build_blas(verts.reshape(-1, 3, 3), nrm, uv, mid, 0, reference_sbvh=True)
    a = orc.OracleScene(tori_scene(refit)).render(threads=8)
    b = orc.OracleScene(tori_scene(fresh)).render(threads=8)
    base = orc.OracleScene(tori_scene(blas)).render(threads=8)
    assert not np.array_equal(a["packed"], base["packed"]), "the deformation must show"
    diff = int((a["packed"] != b["packed"]).sum())
    print(f"{kind} seed {seed} amp {amp}: {diff} differing pixels")
    assert a["stats"] == b["stats"] and util.bit_exact(a["rgb"], b["rgb"]) and diff == 0


def hostile_vertices(pos):
    """Torus soup with hostile vertices in every 23rd triangle, four patterns in turn -> (verts (V, 3), the affected source triangles)."""
    verts = pos.reshape(-1, 3).copy()
    bad = list(range(5, len(pos), 23))
    for j, t in enumerate(bad):
        if j % 4 == 0: verts[3 * t + 1] = (np.nan, np.nan, np.nan)
        elif j % 4 == 1: verts[3 * t, 0] = np.inf
        elif j % 4 == 2: verts[3 * t + 2] = (-np.inf, np.inf, 1.0)
        else: verts[3 * t] = (np.nan, 2.0, -np.inf); verts[3 * t + 1] = (np.nan, np.inf, np.inf); verts[3 * t + 2] = (np.nan, -np.inf, np.nan)
    return verts, bad


def test_hostile_vertices_keep_the_tree_valid_and_the_neighbours_visible():
    import orc
    from pyrtx import host
    blas, pos, nrm, uv, mid = build("Torus", reference_sbvh=True)
    sv = host.slot_vertices(blas)
    verts, bad = hostile_vertices(pos)
    out = host.blas_refit(blas, sv, verts)
    check_refit(blas, out, sv, verts, soup_order=blas.order)
    a = orc.OracleScene(tori_scene(out)).render(threads=8)
    keep = np.setdiff1d(np.arange(len(pos)), bad)                  # the mesh without the affected triangles, freshly built
    fresh = host.build_blas(pos[keep], nrm[keep], uv[keep], mid[keep], 0, reference_sbvh=True)
    b = orc.OracleScene(tori_scene(fresh)).render(threads=8)
    assert a["stats"] == b["stats"] and util.bit_exact(a["rgb"], b["rgb"]) and np.array_equal(a["packed"], b["packed"])
    whole = orc.OracleScene(tori_scene(blas)).render(threads=8)
    assert not np.array_equal(a["packed"], whole["packed"]), "the affected triangles are meant to be in view"


@pytest.mark.parametrize("kind", ["all_nan", "all_inf", "all_equal", "denormal", "huge", "mixed"])
def test_degenerate_vertex_sets(kind):
    from pyrtx import host
    blas, pos, *_ = build("Monkey", reference_sbvh=True)
    sv = host.slot_vertices(blas)
    v = pos.reshape(-1, 3).copy()
    rng = np.random.default_rng(5)
    if kind == "all_nan": v[:] = np.nan
    elif kind == "all_inf": v[:] = np.where(rng.random(v.shape) < 0.5, np.inf, -np.inf)
    elif kind == "all_equal": v[:] = (1.5, -2.0, 0.25)
    elif kind == "denormal": v = (v * f32(1e-41)).astype(f32)
    elif kind == "huge":
        with np.errstate(over="ignore"):
            v = (v * f32(3e38)).astype(f32)                         # overflows to +-inf for most components, FLT_MAX-scale for the rest
    else:
        m = rng.random(v.shape); v[m < 0.1] = np.nan; v[(m > 0.1) & (m < 0.2)] = np.inf; v[(m > 0.2) & (m < 0.3)] = -np.inf; v[(m > 0.3) & (m < 0.35)] = 0.0
    out = host.blas_refit(blas, sv, v)
    reach = check_refit(blas, out, sv, v)
    if kind in ("all_nan", "all_inf"):                             # no finite component anywhere: every leaf is [+0, +0] before the fix
        r = np.array(reach)
        assert (out.nodes["aabb_min"][r] == 0).all() and (out.nodes["aabb_max"][r] == f32(0.005)).all()


def test_argument_checks():
    from pyrtx import host
    blas, pos, *_ = build("Cube", reference_bvh=True)
    sv = host.slot_vertices(blas)
    verts = pos.reshape(-1, 3)
    bad = sv.copy(); bad[3, 1] = len(verts)
    with pytest.raises(ValueError):
        host.blas_refit(blas, bad, verts)
    bad[3, 1] = -1
    with pytest.raises(ValueError):
        host.blas_refit(blas, bad, verts)
    with pytest.raises(ValueError):
        host.blas_refit(blas, sv[:-1], verts)
    with pytest.raises(ValueError):
        host.blas_refit(blas, sv, verts, verts[:-1])
    cyc = copy.copy(blas); cyc.nodes = blas.nodes.copy()
    inner = [i for i in reachable(blas.nodes) if (int(blas.nodes["count"][i]) & 0x3fffffff) == 0]
    cyc.nodes["left_or_first"][inner[-1]] = 0                      # a child pair that leads back to the root
    with pytest.raises(ValueError):
        host.blas_refit(cyc, sv, verts)
    with pytest.raises(ValueError):
        host.slot_vertices(util.sio.Blas(blas.nodes, blas.tri_hot, blas.tri_cold))
