"""tests/layoutset.py — the restatement of the packet layout, the two 4-wide record layouts and the plane lists that the GPU tests compare
the device's read-back layouts with (tests/test_gpu_layouts.py) — on trees written out by hand: the balanced shapes of 5 triangles (both
children of the root are leaves) and of 9 triangles (the left child a leaf of 4, the right child inner: a three-slot record whose third
and fourth slots carry their parent's axis).  The expected records are spelled out here word by word, and every check is shown to fail on
a record with one wrong word.  No GPU, no library."""
import os
import struct
import subprocess

import numpy as np
import pytest

import layoutset as ls
import util
from pyrtx import scene_io as sio

CSRC = os.path.join(util.REPO, "cpu-raytracer_amd", "csrc")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def row(mn, mx, w6, w7):
    """One 8-word row from a box and two integer words."""
    return [bits(mn[0]), bits(mn[1]), bits(mx[0]), bits(mx[1]), bits(mn[2]), bits(mx[2]), w6, w7]


ZERO = [0] * 8
AXIS_X, AXIS_Y, AXIS_Z = 1, 2, 3


def node(mn, mx, left_or_first, count, axis=0):
    return (mn, mx, left_or_first, count | axis << 30)


def tree(slots):
    nodes = np.zeros(len(slots), sio.BVH_NODE)
    for i, s in enumerate(slots):
        if s is None:
            continue
        nodes["aabb_min"][i], nodes["aabb_max"][i] = s[0], s[1]
        nodes["left_or_first"][i] = s[2]
        nodes["count"][i] = np.uint32(s[3]).astype(np.int32)
    return nodes


# boxes: nested, with a -0.0, a repeated plane and a denormal among the coordinates
B5 = {0: ((-2.0, -1.0, -0.0), (3.0, 1.5, 4.0)), 2: ((-2.0, -1.0, 0.5), (0.25, 1.5, 4.0)), 3: ((0.25, -0.5, -0.0), (3.0, 1.0, 1e-40))}
B9 = {0: ((-4.0, -3.0, -2.0), (4.0, 3.0, 2.0)), 2: ((-4.0, -3.0, -2.0), (-1.0, 0.0, 2.0)), 3: ((-1.5, -2.5, -1.0), (4.0, 3.0, 1.75)),
      6: ((-1.5, -2.5, -1.0), (1.0, 3.0, 0.0)), 7: ((0.5, -2.0, -0.5), (4.0, 2.0, 1.75))}


def five():
    """5 triangles: root [0, 5) at slot 0, leaves [0, 2) and [2, 5) at slots 2 and 3, slot 1 unused."""
    return tree([node(*B5[0], 2, 0, AXIS_Y), None, node(*B5[2], 0, 2), node(*B5[3], 2, 3)])


def nine():
    """9 triangles: root at 0; slot 2 the leaf [0, 4); slot 3 inner over [4, 9) with its leaves [4, 6) and [6, 9) at slots 6 and 7; slots 1, 4
    and 5 are holes."""
    return tree([node(*B9[0], 2, 0, AXIS_X), None, node(*B9[2], 0, 4), node(*B9[3], 6, 0, AXIS_Z), None, None, node(*B9[6], 4, 2), node(*B9[7], 6, 3)])


def u32(rows):
    return np.array(rows, np.uint32)


PK5 = u32([row(*B5[0], 2, AXIS_Y << 30), ZERO, row(*B5[2], 0, 2), row(*B5[3], 2, 3)])
PK9 = u32([row(*B9[0], 2, AXIS_X << 30), ZERO, row(*B9[2], 0, 4), row(*B9[3], 6, AXIS_Z << 30), ZERO, ZERO, row(*B9[6], 4, 2), row(*B9[7], 6, 3)])
# closest-hit records: rows 4 .. 7 = the record of the root (its left child is slot 2): a leaf child sits in row 0 / 2 of the record alone
PK4C5 = u32([ZERO] * 4 + [row(*B5[2], 0, 2), ZERO, row(*B5[3], 2, 3), ZERO] + [ZERO] * 4)
PK4C9 = u32([ZERO] * 4
            + [row(*B9[2], 0, 4), ZERO, row(*B9[6], 4, 2 | AXIS_Z << 26), row(*B9[7], 6, 3)]      # the root: leaf 2 | the children of node 3, its axis in the first
            + [ZERO] * 4
            + [row(*B9[6], 4, 2), ZERO, row(*B9[7], 6, 3), ZERO]                                # node 3 (left child 6): two leaf children, no parent axis
            + [ZERO] * 4)
# shadow-ray records: the same slot nodes without axis fields, used slots first, in a schedule's order (here: largest box first)
PK45 = u32([ZERO] * 4 + [row(*B5[2], 0, 2), row(*B5[3], 2, 3), ZERO, ZERO] + [ZERO] * 4)
PK49 = u32([ZERO] * 4 + [row(*B9[2], 0, 4), row(*B9[7], 6, 3), row(*B9[6], 4, 2), ZERO] + [ZERO] * 4 + [row(*B9[7], 6, 3), row(*B9[6], 4, 2), ZERO, ZERO] + [ZERO] * 4)

CASES = {"five": (five, PK5, PK4C5, PK45), "nine": (nine, PK9, PK4C9, PK49)}


def plane_list(nodes, axis):
    """The list the device would hold: min and max of every slot, in the radix sort's order (sign-magnitude key: -0.0 before +0.0)."""
    v = np.concatenate([nodes["aabb_min"][:, axis], nodes["aabb_max"][:, axis]]).astype(np.float32).view(np.uint32)
    key = np.where(v & 0x80000000, ~v, v | 0x80000000).astype(np.uint32)
    return v[np.argsort(key, kind="stable")]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_gives_the_records_written_out_by_hand(name):
    make, pk, pk4c, pk4 = CASES[name]
    nodes = make()
    assert ls.reachable(nodes).tolist() == [i in ((0, 2, 3) if name == "five" else (0, 2, 3, 6, 7)) for i in range(len(nodes))]
    assert np.array_equal(ls.pk(nodes), pk)
    assert np.array_equal(ls.pk4c(nodes), pk4c) and pk4c.shape == (2 * len(nodes) + 4, 8)
    ls.check_pk(nodes, pk); ls.check_pk4c(nodes, pk4c); ls.check_pk4(nodes, pk4); ls.check_pk4(nodes, pk4, pk4.copy())
    for order in ([1, 0, 2, 3], [2, 0, 1, 3], [3, 2, 1, 0]):         # the slot order is a schedule: any order of the root's record passes
        moved = pk4.copy(); moved[4:8] = pk4[4:8][order]
        ls.check_pk4(nodes, moved)
    for a in range(3):
        got = plane_list(nodes, a)
        assert len(got) == 2 * len(nodes)
        ls.check_planes(nodes, a, got)
    ls.check_blas(nodes, {"pk": pk, "pk4": pk4, "pk4c": pk4c, "planes": [plane_list(nodes, a) for a in range(3)]})
    ls.check_blas(nodes, {"pk": pk, "pk4": None, "pk4c": None, "planes": [plane_list(nodes, a) for a in range(3)]})


def test_signed_zeros_and_nan_in_the_plane_lists():
    nodes = five()
    z = plane_list(nodes, 2)
    assert list(z[:4]) == [0x80000000, 0x80000000, 0, 0], "two -0.0 (root and slot 3), then the two +0.0 of the unused slot"
    ls.check_planes(nodes, 2, z)
    nodes["aabb_max"][1][0] = np.nan                                    # an unreachable slot's NaN becomes +inf, and still counts
    want = plane_list(nodes, 0)
    assert want[-1] == 0x7fc00000
    with pytest.raises(AssertionError):
        ls.check_planes(nodes, 0, want)
    want[-1] = 0x7f800000
    ls.check_planes(nodes, 0, want)


def fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


@pytest.mark.parametrize("name", list(CASES))
def test_every_check_bites_on_one_wrong_word(name):
    make, pk, pk4c, pk4 = CASES[name]
    nodes = make()

    def wrong(a, r, w, v=None):
        b = a.copy(); b[r, w] = (b[r, w] ^ 1) if v is None else v
        return b
    # pk: a box float of a reachable node, its first word, its axis bits; an unreachable slot that is not what it was
    fails(ls.check_pk, nodes, wrong(pk, 3, 2)); fails(ls.check_pk, nodes, wrong(pk, 2, 6)); fails(ls.check_pk, nodes, wrong(pk, 0, 7, 3 << 30))
    fails(ls.check_pk, nodes, wrong(pk, 1, 0))
    before = pk.copy(); before[1] = 7
    ls.check_pk(nodes, before, before); fails(ls.check_pk, nodes, pk, before)
    # pk4c: a box float, a first word, a leaf count, the parent-axis field, the slot-axis field, an unused slot, the tail
    fails(ls.check_pk4c, nodes, wrong(pk4c, 4, 4)); fails(ls.check_pk4c, nodes, wrong(pk4c, 6, 6)); fails(ls.check_pk4c, nodes, wrong(pk4c, 6, 7))
    fails(ls.check_pk4c, nodes, wrong(pk4c, 6, 7, int(pk4c[6, 7]) ^ (1 << 26)))
    fails(ls.check_pk4c, nodes, wrong(pk4c, 6, 7, int(pk4c[6, 7]) ^ (2 << 26)))
    fails(ls.check_pk4c, nodes, wrong(pk4c, 4, 7, int(pk4c[4, 7]) | (1 << 30)))
    fails(ls.check_pk4c, nodes, wrong(pk4c, 5, 0)); fails(ls.check_pk4c, nodes, wrong(pk4c, len(pk4c) - 1, 3))
    if name == "nine":
        assert (int(pk4c[6, 7]) >> 26) & 3 == AXIS_Z and (int(pk4c[12, 7]) >> 26) & 3 == 0
        fails(ls.check_pk4c, nodes, wrong(pk4c, 12, 7, int(pk4c[12, 7]) | (AXIS_Z << 26)))      # node 6 as a child of node 3 carries no parent axis
    # pk4: a box float, a first word, a leaf count, a slot named twice, a missing slot, a stale unused slot, changed topology words
    fails(ls.check_pk4, nodes, wrong(pk4, 5, 1)); fails(ls.check_pk4, nodes, wrong(pk4, 5, 6)); fails(ls.check_pk4, nodes, wrong(pk4, 4, 7))
    twice = pk4.copy(); twice[5] = twice[4]
    fails(ls.check_pk4, nodes, twice)
    fails(ls.check_pk4, nodes, wrong(pk4, 5, slice(None), 0))
    fails(ls.check_pk4, nodes, wrong(pk4, 7, 5)); fails(ls.check_pk4, nodes, wrong(pk4, 0, 0))
    swapped = pk4.copy(); swapped[[4, 5]] = pk4[[5, 4]]
    ls.check_pk4(nodes, swapped); fails(ls.check_pk4, nodes, swapped, pk4)                     # a right record in another order than before the call
    # a box in the wrong slot: the boxes of two slots exchanged, their topology words kept
    crossed = pk4.copy(); crossed[4, :6] = pk4[5, :6]; crossed[5, :6] = pk4[4, :6]
    fails(ls.check_pk4, nodes, crossed)
    # planes: one entry missing (replaced by a copy of its neighbour), two entries exchanged, a short list
    for a in range(3):
        good = plane_list(nodes, a)
        lost = good.copy(); k = int(np.flatnonzero(good[1:] != good[:-1])[0]); lost[k + 1] = lost[k]
        fails(ls.check_planes, nodes, a, lost)
        k = int(np.flatnonzero(good[1:].view(np.float32) > good[:-1].view(np.float32))[0])
        swapped = good.copy(); swapped[[k, k + 1]] = good[[k + 1, k]]
        fails(ls.check_planes, nodes, a, swapped)
        fails(ls.check_planes, nodes, a, good[:-1])


def test_layout_check_passes():
    """csrc/layout_check.cpp: the record writers of csrc/rtx_layout.h and the host converters of csrc/rtx_layout_host.h against records spelled
    out by hand (the rows above, as C literals), the lane record's round trip, and the finish pass of a refit and a build run on the host
    over converted trees.  A stand-alone program built with the host compiler under -fsanitize=address,undefined; nothing is loaded into
    Python and no GPU is needed."""
    out = subprocess.run(["make", "-B", "-C", CSRC, "layout_check"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "layout_check: ok" in out.stdout.splitlines(), out.stdout[-4000:]
    assert "FAILED" not in out.stdout
