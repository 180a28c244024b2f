"""The node layouts the kernels walk, restated in numpy as functions of the lane layout alone (read-back rtx_bvh_node arrays: aabb_min,
aabb_max, left_or_first, count), from the record formats documented above convert_nodes_pk, build_nodes_pk4 and build_nodes_pk4c in
csrc/rtx_api.hip.  Nothing here calls the library; everything is compared as uint32 bit patterns, a row of 8 words per node or record slot:

  row    (min.x, min.y, max.x, max.y, min.z, max.z, W6, W7)
  pk     one row per node slot: W6 = left_or_first, W7 = count (axis bits included)
  pk4c   closest-hit 4-wide records: 4 rows at row 2 * left of every reachable inner node j (left = j's left child): rows 0-1 the left
         child's children (or the left child itself, a leaf, in row 0), rows 2-3 the right child's; W6 = the slot node's left_or_first,
         W7 = leaf count | axis of the slot's parent << 26 (rows 0 and 2, only when that parent is an inner child of j) | axis of the slot
         node << 30; every other row is zero bytes
  pk4    shadow-ray 4-wide records: the same place and the same slot nodes, W7 = leaf count without axis bits, in an order that is a
         schedule fixed at upload (not restated); every other row is zero bytes
  planes per axis 2 * node_count floats: every slot's min and max on that axis, NaN -> +inf, sorted ascending by the radix sort's order
         (-0.0 before +0.0)
The Python loops are linear in the node count (one stack walk); the rest is array arithmetic.
"""
import numpy as np

COUNT_MASK = 0x3fffffff
PINF = 0x7f800000


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def reachable(nodes):
    """Boolean mask of the node slots a traversal from the root reaches."""
    n = len(nodes)
    left = nodes["left_or_first"].astype(np.int64)
    leaf = (nodes["count"].astype(np.int64) & COUNT_MASK) > 0
    mask = np.zeros(n, bool)
    stack = [0]
    while stack:
        i = stack.pop()
        assert 0 <= i < n and not mask[i], f"node {i}: outside the array or reached twice"
        mask[i] = True
        if not leaf[i]:
            stack.append(int(left[i])); stack.append(int(left[i]) + 1)
    return mask


def _rows(nodes, w6, w7):
    mn, mx = _u32(nodes["aabb_min"]).reshape(-1, 3), _u32(nodes["aabb_max"]).reshape(-1, 3)
    return np.stack([mn[:, 0], mn[:, 1], mx[:, 0], mx[:, 1], mn[:, 2], mx[:, 2], w6.astype(np.uint32), w7.astype(np.uint32)], axis=1)


def pk(nodes):
    """(n, 8) uint32: the packet layout of every slot (convert_nodes_pk)."""
    return _rows(nodes, _u32(nodes["left_or_first"]), _u32(nodes["count"]))


def check_pk(nodes, got, before=None):
    """Reachable slots hold pk(nodes) exactly; unreachable slots (holes, index 1) hold what `before` held — zero bytes when before is None."""
    want = pk(nodes)
    assert got.shape == want.shape and got.dtype == np.uint32, (got.shape, want.shape)
    r = reachable(nodes)
    bad = np.flatnonzero(r & (got != want).any(1))
    assert not len(bad), f"pk: reachable node {bad[0]} holds {got[bad[0]]}, the lane layout gives {want[bad[0]]} ({len(bad)} nodes differ)"
    old = np.zeros_like(want) if before is None else before
    bad = np.flatnonzero(~r & (got != old).any(1))
    assert not len(bad), f"pk: unreachable slot {bad[0]} holds {got[bad[0]]}, it held {old[bad[0]]} ({len(bad)} slots differ)"


def _slot_nodes(nodes):
    """-> (J, L, S): reachable inner nodes, their left-child indices, and S (len(J), 4) = the node in each tree-ordered record slot
    (slots 0-1 under the left child, 2-3 under the right one), -1 for an unused slot; P (len(J), 4) = that slot's parent when the parent
    is an inner child of the record's node and the slot is its first, else -1."""
    left = nodes["left_or_first"].astype(np.int64)
    cnt = nodes["count"].astype(np.int64) & COUNT_MASK
    J = np.flatnonzero(reachable(nodes) & (cnt == 0))
    L = left[J]
    S = np.full((len(J), 4), -1, np.int64); P = np.full((len(J), 4), -1, np.int64)
    for g in range(2):
        c = L + g
        is_leaf = cnt[c] > 0
        S[:, 2 * g] = np.where(is_leaf, c, left[c])
        S[:, 2 * g + 1] = np.where(is_leaf, -1, left[c] + 1)
        P[:, 2 * g] = np.where(is_leaf, -1, c)
    return J, L, S, P


def pk4c(nodes):
    """(2n + 4, 8) uint32: the closest-hit 4-wide records (build_nodes_pk4c), meta words included; zero bytes everywhere else."""
    n = len(nodes)
    out = np.zeros((2 * n + 4, 8), np.uint32)
    J, L, S, P = _slot_nodes(nodes)
    if not len(J):
        return out
    count = _u32(nodes["count"]).astype(np.int64)
    used = S >= 0
    si = np.where(used, S, 0)
    parent_axis = np.where(P >= 0, count[np.where(P >= 0, P, 0)] >> 30, 0)
    meta = (count[si] & COUNT_MASK) | ((count[si] >> 30) << 30) | (parent_axis << 26)
    rows = _rows(nodes, _u32(nodes["left_or_first"]), np.zeros(n, np.uint32))[si]       # (len(J), 4, 8)
    rows[:, :, 7] = meta.astype(np.uint32)
    rows[~used] = 0
    at = (2 * L)[:, None] + np.arange(4)[None, :]
    out[at.reshape(-1)] = rows.reshape(-1, 8)
    return out


def check_pk4c(nodes, got):
    want = pk4c(nodes)
    assert got.shape == want.shape and got.dtype == np.uint32, (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), (f"pk4c: record slot {bad[0]} (record of left child {bad[0] // 4 * 2}, slot {bad[0] % 4}) holds "
                          f"{[hex(int(w)) for w in got[bad[0]]]}, the lane layout gives {[hex(int(w)) for w in want[bad[0]]]} ({len(bad)} slots differ)")


def check_pk4(nodes, records, before=None):
    """The shadow-ray 4-wide records against the lane layout, whatever their slot order.  For every reachable inner node the used slots'
    (first, leaf count) words name exactly its grandchildren (a leaf child itself), each once; each slot's six box floats are that node's
    box bit for bit; every other slot is zero bytes.  before: the records from before a call that keeps the topology — then every slot's two
    topology words are also unchanged."""
    n = len(nodes)
    assert records.shape == (2 * n + 4, 8) and records.dtype == np.uint32, records.shape
    J, L, S, _ = _slot_nodes(nodes)
    rest = np.ones(2 * n + 4, bool)
    if len(J):
        used = S >= 0
        si = np.where(used, S, 0)
        want = _rows(nodes, _u32(nodes["left_or_first"]), _u32(nodes["count"]) & np.uint32(COUNT_MASK))[si]
        want[~used] = 0
        at = (2 * L)[:, None] + np.arange(4)[None, :]
        got = records[at]                                               # (len(J), 4, 8)
        rest[at.reshape(-1)] = False
        key = lambda r: (r[:, :, 6].astype(np.uint64) << np.uint64(32)) | r[:, :, 7].astype(np.uint64)     # unused slots: key 0, first
        kw, kg = key(want), key(got)
        ow, og = np.argsort(kw, axis=1, kind="stable"), np.argsort(kg, axis=1, kind="stable")
        sw, sg = np.take_along_axis(kw, ow, 1), np.take_along_axis(kg, og, 1)
        bad = np.flatnonzero((sw != sg).any(1))
        assert not len(bad), (f"pk4: the record of node {J[bad[0]]} names (first, count) {[(int(k >> np.uint64(32)), int(k & np.uint64(0xffffffff))) for k in sg[bad[0]]]}, "
                              f"its grandchildren are {[(int(k >> np.uint64(32)), int(k & np.uint64(0xffffffff))) for k in sw[bad[0]]]} ({len(bad)} records differ)")
        assert (sw[:, 1:][sw[:, 1:] != 0] != sw[:, :-1][sw[:, 1:] != 0]).all(), "two slot nodes of one record share their (first, count) words"
        gw = np.take_along_axis(want, ow[:, :, None], 1); gg = np.take_along_axis(got, og[:, :, None], 1)
        bad = np.argwhere((gw != gg).any(2))
        assert not len(bad), (f"pk4: in the record of node {J[bad[0][0]]} the slot of (first, count) {tuple(int(w) for w in gg[bad[0][0], bad[0][1], 6:])} holds the box "
                              f"{gg[bad[0][0], bad[0][1], :6]}, the node's is {gw[bad[0][0], bad[0][1], :6]} ({len(bad)} slots differ)")
    bad = np.flatnonzero(rest & (records != 0).any(1))
    assert not len(bad), f"pk4: slot {bad[0]} belongs to no reachable record and is not zero bytes ({len(bad)} slots)"
    if before is not None:
        assert before.shape == records.shape
        bad = np.flatnonzero((before[:, 6:] != records[:, 6:]).any(1))
        assert not len(bad), f"pk4: slot {bad[0]}'s topology words changed from {before[bad[0], 6:]} to {records[bad[0], 6:]} ({len(bad)} slots)"


def planes(nodes, axis):
    """The multiset of bit patterns a bound mesh's plane list of `axis` holds, as a sorted uint32 array of 2 * node_count entries: every
    slot's min and max on that axis, unreachable slots included, NaN replaced by +inf."""
    v = np.concatenate([nodes["aabb_min"][:, axis], nodes["aabb_max"][:, axis]]).astype(np.float32)
    bits = _u32(v).copy()
    bits[np.isnan(v)] = PINF
    return np.sort(bits)


def check_planes(nodes, axis, got):
    """got: the read-back list as uint32 bit patterns.  Multiset plus monotonicity, not np.sort of floats: the radix sort puts -0.0 before
    +0.0, numpy leaves them in any order."""
    want = planes(nodes, axis)
    assert got.shape == want.shape and got.dtype == np.uint32, (axis, got.shape, want.shape)
    if not np.array_equal(np.sort(got), want):
        a, b = np.unique(got), np.unique(want)
        raise AssertionError(f"planes[{axis}]: bit patterns only in the list {[hex(int(x)) for x in np.setdiff1d(a, b)[:4]]}, only in the nodes "
                             f"{[hex(int(x)) for x in np.setdiff1d(b, a)[:4]]} (or the same patterns in other numbers)")
    f = got.view(np.float32)
    assert not np.isnan(f).any(), f"planes[{axis}]: a NaN in the list"
    bad = np.flatnonzero(~(f[:-1] <= f[1:]))
    assert not len(bad), f"planes[{axis}]: entry {bad[0]} ({f[bad[0]]}) is above entry {bad[0] + 1} ({f[bad[0] + 1]})"


def check_blas(nodes, lay, pk_before=None, pk4_before=None, bound=True):
    """Everything a mesh's read-back layouts (Renderer.debug_read_layouts) must satisfy on the read-back nodes of the same state."""
    check_pk(nodes, lay["pk"], pk_before)
    if lay["pk4"] is not None:
        check_pk4(nodes, lay["pk4"], pk4_before)
    if lay["pk4c"] is not None:
        check_pk4c(nodes, lay["pk4c"])
    if bound:
        for a in range(3):
            check_planes(nodes, a, lay["planes"][a])
