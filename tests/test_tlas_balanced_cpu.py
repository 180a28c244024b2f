"""The balanced TLAS of rtx_update_instances on the CPU: rtxh_tlas_build_balanced is the code the kernels run (csrc/rtx_update_math.h) driven
sequentially, so what holds here is what the device tree is compared with bit for bit (tests/test_gpu_update_instances.py).

Checked for every input: the indices are a permutation, every leaf box is its instance's box after AABB::fix_if_needed, the split-axis bits
are 1..3, a NaN inner box covers only instances whose own box is not finite, the deepest inner node sits at the closed-form depth ceil(log2 n) - 1, holes are zero, two runs give the same bytes; for finite
input also that every inner node's stored box encloses its children's stored boxes componentwise.  The bounds are not measured: they are
the properties the host relies on before any kernel runs (validate_references, the packet-stack rule of plan_stack_limits, csrc/rtx_plan.h).
"""
import ctypes as C

import numpy as np
import pytest

import util
from pyrtx import host, scene_io as sio

f32 = np.float32


def fix_if_needed(mn, mx):                  # AABB::fix_if_needed, AABB.h:26-32, in fp32
    mn = np.array(mn, f32); mx = np.array(mx, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            if f32(mx[a] - mn[a]) < f32(0.001):
                mx[a] = f32(mx[a] + f32(0.005))
    return mn, mx


def same_bits(a, b):
    """fp32 values equal bit for bit; two NaNs count as equal (x86 and gfx950 generate different default NaNs, util.bit_exact)."""
    return util.bit_exact(a, b)


def check_tree(nodes, idx, aabbs, finite):
    """The properties above; returns the depth of the deepest inner node (-1: the root is a leaf)."""
    n = len(idx)
    assert len(nodes) == host.tlas_balanced_node_count(n) == 2 << int(np.ceil(np.log2(n))) if n > 1 else len(nodes) == 2
    assert np.array_equal(np.sort(idx), np.arange(n, dtype=np.int32)), "indices are not a permutation"
    seen = np.zeros(len(nodes), bool)
    covered = np.zeros(n, np.int32)
    deepest = -1
    stack = [(0, 0)]
    while stack:
        i, d = stack.pop()
        assert 0 <= i < len(nodes) and i != 1 and not seen[i]
        seen[i] = True
        cnt, first = int(nodes["count"][i]) & 0x3FFFFFFF, int(nodes["left_or_first"][i])
        if cnt > 0:
            assert cnt == 1 and 0 <= first < n and (int(nodes["count"][i]) >> 30) & 3 == 0
            covered[first] += 1
            mn, mx = fix_if_needed(aabbs[idx[first], :3], aabbs[idx[first], 3:])
            assert same_bits(nodes["aabb_min"][i], mn) and same_bits(nodes["aabb_max"][i], mx), ("leaf box", i)
        else:
            assert ((int(nodes["count"][i]) >> 30) & 3) in (1, 2, 3), ("axis bits", i)
            assert 2 <= first and first + 1 < len(nodes), ("child range", i)
            deepest = max(deepest, d)
            if finite:
                for ch in (first, first + 1):
                    assert np.all(nodes["aabb_min"][i] <= nodes["aabb_min"][ch]) and np.all(nodes["aabb_max"][i] >= nodes["aabb_max"][ch]), ("enclosure", i, ch)
            stack.append((first, d + 1)); stack.append((first + 1, d + 1))
            if np.isnan(nodes["aabb_min"][i]).any() or np.isnan(nodes["aabb_max"][i]).any():
                # a NaN inner box covers instances with a non-finite box only: a bad pose never hides a neighbour (sort_key, bit 46)
                sub, leaves = [first, first + 1], []
                while sub:
                    k = sub.pop()
                    if int(nodes["count"][k]) & 0x3FFFFFFF:
                        leaves.append(int(nodes["left_or_first"][k]))
                    else:
                        sub += [int(nodes["left_or_first"][k]), int(nodes["left_or_first"][k]) + 1]
                assert not any(np.isfinite(aabbs[idx[s]]).all() for s in leaves), ("NaN inner box over a finite instance", i)
    assert np.all(covered == 1), "every sorted slot belongs to exactly one leaf"
    assert not nodes[~seen].tobytes().strip(b"\0"), "slots that are no node must be zero"
    return deepest


def build_checked(pos, aabbs, finite=True):
    pos = np.ascontiguousarray(pos, f32); aabbs = np.ascontiguousarray(aabbs, f32)
    n = len(pos)
    nodes, idx = host.tlas_build_balanced(pos, aabbs)
    again, idx2 = host.tlas_build_balanced(pos.copy(), aabbs.copy())
    assert nodes.tobytes() == again.tobytes() and idx.tobytes() == idx2.tobytes(), "two runs differ"
    depth = check_tree(nodes, idx, aabbs, finite)
    want = -1 if n == 1 else int(np.ceil(np.log2(n))) - 1
    assert depth == want == host.tlas_balanced_inner_depth(n), (n, depth, want)
    return nodes, idx


def cloud(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-spread, spread, (n, 3)).astype(f32)
    half = rng.uniform(0.1, 2.0, (n, 3)).astype(f32)
    return pos, np.concatenate([pos - half, pos + half], axis=1).astype(f32)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 65536])
def test_seeded_clouds(n):
    pos, aabbs = cloud(n, 1000 + n)
    nodes, idx = build_checked(pos, aabbs)
    if n >= 64:      # the order is spatial: the two halves under the root are separated on the root's axis more often than not
        axis = ((int(nodes["count"][0]) >> 30) & 3) - 1
        l, r = int(nodes["left_or_first"][0]), int(nodes["left_or_first"][0]) + 1
        assert nodes["aabb_min"][l][axis] + nodes["aabb_max"][l][axis] <= nodes["aabb_min"][r][axis] + nodes["aabb_max"][r][axis]


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 65536])
@pytest.mark.parametrize("kind", ["all_equal", "collinear", "duplicates", "zero_extent", "huge"])
def test_adversarial_finite_sets(kind, n):
    rng = np.random.default_rng(7 * n + len(kind))
    if kind == "all_equal":
        pos = np.tile(np.array([[1.5, -2.0, 3.25]], f32), (n, 1))
    elif kind == "collinear":
        pos = np.zeros((n, 3), f32); pos[:, 1] = np.linspace(-5, 5, n, dtype=f32)
    elif kind == "duplicates":
        pos = rng.uniform(-3, 3, (max(1, n // 4), 3)).astype(f32)[rng.integers(0, max(1, n // 4), n)]
    elif kind == "zero_extent":
        pos = rng.uniform(-3, 3, (n, 3)).astype(f32)
    else:
        pos = (rng.uniform(-1, 1, (n, 3)) * 1e30).astype(f32); pos[0] = 3e38; pos[-1] = -3e38     # hi - lo overflows
    half = np.zeros((n, 3), f32) if kind == "zero_extent" else rng.uniform(0.1, 1.0, (n, 3)).astype(f32)
    with np.errstate(over="ignore"):
        aabbs = np.concatenate([pos - half, pos + half], axis=1).astype(f32)
    build_checked(pos, aabbs, finite=bool(np.isfinite(aabbs).all()))


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 65536])
def test_nan_and_inf_positions_and_boxes(n):
    """Non-finite input: the tree stays a valid tree (permutation, ranges, depth, leaf boxes, determinism); enclosure is not asked of NaN."""
    pos, aabbs = cloud(n, 99 + n)
    rng = np.random.default_rng(n)
    for k, v in enumerate([np.nan, np.inf, -np.inf, np.nan]):
        i = int(rng.integers(0, n))
        pos[i, k % 3] = v
        aabbs[int(rng.integers(0, n)), int(rng.integers(0, 6))] = v
    nodes, idx = build_checked(pos, aabbs, finite=False)
    bad = ~np.isfinite(aabbs).all(axis=1)
    assert bad[idx[:bad.sum()]].all() and not bad[idx[bad.sum():]].any(), "instances with a non-finite box sort first"
    build_checked(np.full((n, 3), np.nan, f32), np.full((n, 6), np.nan, f32), finite=False)
    build_checked(np.full((n, 3), np.inf, f32), aabbs, finite=False)


def poses(name, frames, delta=0.0166666667):
    """Positions / rotations of golden `name` after `frames` updates (Scene.cpp:141-155), as test_dynamic_frames steps them."""
    from test_dynamic_frames import animate, initial_state
    pos, rot = initial_state("dynamic" if name == "dynamic" else "tori16")
    time = f32(0.0)
    for _ in range(frames):
        time = animate(pos, rot, time, delta)
    return np.array(pos, f32), np.array(rot, f32)


@pytest.mark.parametrize("name,frames", [("dynamic", 3), ("tori16", 2), ("tori16_f1", 1)])
def test_golden_frame_states(name, frames):
    """rtxh_scene_update_balanced = rtx_update_instances on the host: its instance records are the REAL reference's (the goldens' frame
    state) bit for bit — the kernels' restatement of Mesh::update — and its tree over them has every property above."""
    sc, _ = util.load_golden(name)
    pos, rot = poses(name, frames)
    inst, nodes, idx = host.scene_update_balanced(sc, pos, rot)
    assert inst.tobytes() == np.ascontiguousarray(sc.instances).tobytes()
    aabbs = np.zeros((len(pos), 6), f32)
    for i in range(len(pos)):
        root = sc.blas[sc.instances["blas_id"][i]].nodes[0]
        _, mn, mx = host.instance_update(pos[i], rot[i], root["aabb_min"], root["aabb_max"], 0)
        aabbs[i, :3] = mn; aabbs[i, 3:] = mx
    n2, i2 = build_checked(pos, aabbs)
    assert nodes.tobytes() == n2.tobytes() and idx.tobytes() == i2.tobytes()


@pytest.mark.parametrize("name,frames", [("dynamic", 3), ("tori16", 2)])
def test_oracle_frame_with_balanced_tree_is_the_reference_golden(name, frames):
    """The tree decides only which of two exactly tied hits is found first: with the balanced tree in place of the reference-built one the
    oracle renders the reference's golden frame, identical in every pixel and ray count."""
    import orc
    sc, g = util.load_golden(name)
    pos, rot = poses(name, frames)
    sc.instances, sc.tlas_nodes, sc.tlas_indices = host.scene_update_balanced(sc, pos, rot)
    out = orc.OracleScene(sc).render(threads=8)
    cmp = util.compare_to_golden(out, g)
    print(name, cmp)
    assert cmp["stats_equal"] and cmp["nan_mismatch"] == 0 and cmp["max_abs"] == 0.0 and cmp["n_diff_pixels"] == 0 and cmp["packed_mismatch"] == 0, cmp


def left_first_fraction(nodes):
    """Share of the inner nodes whose left child's box centre is not beyond the right child's on the node's stored axis."""
    inner = np.flatnonzero(((nodes["count"] & 0x3FFFFFFF) == 0) & ((nodes["count"] >> 30) & 3 != 0))
    axis = ((nodes["count"][inner] >> 30) & 3) - 1
    l = nodes["left_or_first"][inner]
    cl = nodes["aabb_min"][l, axis] + nodes["aabb_max"][l, axis]
    cr = nodes["aabb_min"][l + 1, axis] + nodes["aabb_max"][l + 1, axis]
    return float((cl <= cr).mean()), len(inner)


@pytest.mark.parametrize("n", [64, 1000, 65536])
def test_stored_axis_has_the_left_child_first(n):
    """BVHNode::should_visit_left_first reads the stored axis as "the left child is the nearer one for a ray travelling in +axis".  The
    topology is fixed, so the builder cannot swap children; it stores the axis with the largest signed (right - left) centre difference,
    and the claim holds at a node unless the right centre is smaller on ALL three axes.  Floor: for two halves drawn independently of the
    order (no spatial sort at all) each axis is the wrong way round with probability 1/2, all three with 1/8, so 7/8 of the nodes hold; a
    Morton order must do at least that well, and for a node over two leaves with different codes it holds always (the first differing
    code bit is an axis on which left < right)."""
    pos, aabbs = cloud(n, 4000 + n)
    nodes, _ = host.tlas_build_balanced(pos, aabbs)
    frac, count = left_first_fraction(nodes)
    print(f"n = {n}: left child first on the stored axis at {frac:.4f} of {count} inner nodes")
    assert count == n - 1 and frac >= 7 / 8


def test_every_instance_count_has_a_valid_shape():
    """The shape alone, for every n a small scene can have and a spread of large ones: all-equal boxes, so only ranges and depth matter."""
    for n in list(range(1, 130)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4097, 32767, 32769, 65535]:
        pos = np.zeros((n, 3), f32); aabbs = np.tile(np.array([[-1, -1, -1, 1, 1, 1]], f32), (n, 1))
        nodes, idx = host.tlas_build_balanced(pos, aabbs)
        assert np.array_equal(idx, np.arange(n)), n            # equal codes: the index breaks the tie, the order is total
        assert check_tree(nodes, idx, aabbs, True) == host.tlas_balanced_inner_depth(n), n


def test_limits_and_argument_checks():
    L = host.lib()
    nc = C.c_int32()
    one = np.zeros(6, f32)
    assert L.rtxh_tlas_build_balanced(0, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, C.byref(nc)) == 1
    assert L.rtxh_tlas_build_balanced(1, None, one.ctypes.data, one.ctypes.data, one.ctypes.data, C.byref(nc)) == 1
    assert L.rtxh_tlas_build_balanced(65537, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, C.byref(nc)) == 4
    assert host.tlas_balanced_node_count(65536) == 131072 and host.tlas_balanced_node_count(65537) == 0 and host.tlas_balanced_node_count(0) == 0
    assert [host.tlas_balanced_inner_depth(n) for n in (1, 2, 3, 4, 5, 16, 17, 576, 65536)] == [-1, 0, 1, 1, 2, 3, 4, 9, 15]


def test_abi_entry_points_exist_and_check_their_arguments():
    """include/rtx.h: rtx_update_instances / rtx_read_frame_state are exported, bound by pyrtx.api, and refuse a null context without
    touching a device (the checks that need a context run on the GPU: tests/test_gpu_update_instances.py)."""
    from pyrtx import api
    lib = api.load_library()
    for name in api.UPDATE_EXPORTS:
        assert hasattr(lib, name) and name in api.EXPORTS, name
    four = np.zeros(4, f32)
    assert lib.rtx_update_instances(None, four.ctypes.data, four.ctypes.data, 1) == 1
    assert lib.rtx_read_frame_state(None, None, None, None, None) == 1
    assert hasattr(api.Renderer, "update_instances") and hasattr(api.Renderer, "read_frame_state")
    assert api.RTX_UPDATE_MAX_INSTANCES == 65536
