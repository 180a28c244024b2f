"""The second round of a filtered walk query: what a call of more than RTX_QUERY_CHUNK_RAYS rows reads and writes at its round's offset — the
row masks, the signed distance and the feature code, the K entries per row of a listed channel, the count.

Per query kind a base set of R = 4097 rows from the kind's generator (pointset, hitset, sweepset, boxset) in the mixed frame of sideset.py
(two meshes, two spheres, a plane; one mask bit per object), with per-row masks drawn from a seeded generator, answered once by the host twin.
On the device rows and masks are tiled to N = RTX_QUERY_CHUNK_RAYS + 3 by i mod R: 2^20 mod 4097 = 3841, so row CHUNK + j carries base row
3841 + j, and a round that read its masks or wrote its outputs without its offset gives other rows.  Every comparison is bit for bit against
the twin's answers indexed by i mod R.  test_a_wrong_offset_would_show (no GPU) is the condition: at least a quarter of the base rows change
their twin answer under the masks of base row (r + 3841) mod R."""
import functools

import numpy as np
import pytest

import boxset
import hitset
import pointset
import sideset as ss
import sweepset

gpu = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
R = 4097
CHUNK = 1 << 20                                                                # RTX_QUERY_CHUNK_RAYS
SHIFT = CHUNK % R
N = CHUNK + 3
OBJECT_MASKS = np.array([1, 2, 4, 8, 16], u32)                                 # icosphere, Diamond, two spheres, the plane
MASK_SEED = 5
KINDS = ("nearest", "signed", "hits", "sweep", "overlap")


@functools.lru_cache(maxsize=None)
def frame():
    return ss.rules_scene()


@functools.lru_cache(maxsize=None)
def row_masks():
    """(R,) uint32 over the five object bits, an eighth of them 0: not all alike, and some objects hidden from most rows."""
    rng = np.random.default_rng(MASK_SEED)
    m = rng.integers(1, 32, R).astype(u32)
    m[rng.integers(0, 8, R) == 0] = 0
    assert len(np.unique(m)) == 32 and ((m & 31) != 31).sum() > R // 2
    return m


@functools.lru_cache(maxsize=None)
def base_rows(kind):
    """R rows of the kind's generator: more than R generated, R of them drawn by a seeded permutation (every class stays present)."""
    sc, _ = frame()
    gen = {"nearest": lambda: pointset.generate(sc, 5200, 41), "signed": lambda: pointset.generate(sc, 5200, 43), "hits": lambda: hitset.generate(sc, 400, 41),
           "sweep": lambda: sweepset.generate(sc, 4800, 41), "overlap": lambda: boxset.generate(sc, 330, 41)}[kind]
    rows = gen()[0]
    assert len(rows) >= R, (kind, len(rows))
    return np.ascontiguousarray(rows[np.sort(np.random.default_rng(7).permutation(len(rows))[:R])], f32)


def twin(kind, masks):
    """The host twin's answers for the base rows under per-row `masks`: {output: array}, the outputs the device tests compare."""
    from pyrtx import host
    sc, meshes = frame()
    rows, kw = base_rows(kind), dict(mask=masks, object_masks=OBJECT_MASKS)
    if kind == "nearest":
        out = host.query_nearest(sc, rows, ("distance", "object_id"), **kw)
    elif kind == "signed":
        out = host.query_signed_distance(sc, rows, ("distance",), pseudonormals=ss.host_tables(meshes), **kw)
    elif kind == "hits":
        out = host.query_hits(sc, rows, 2, ("distance", "triangle_id"), True, **kw)
    elif kind == "sweep":
        out = host.query_sweep(sc, rows, ("distance", "object_id"), **kw)
    else:
        out = host.query_overlap(sc, rows, 2, True, **kw)
        out["any"] = host.query_overlapped(sc, rows, **kw)
    out.pop("stack_max", None)
    return out


@functools.lru_cache(maxsize=None)
def expected(kind):
    return twin(kind, row_masks())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32, copy=False)


@pytest.mark.parametrize("kind", KINDS)
def test_a_wrong_offset_would_show(kind):
    """From the twins alone: under the masks of base row (r + SHIFT) mod R at least a quarter of the rows answer otherwise."""
    assert SHIFT == 3841
    want, other = expected(kind), twin(kind, np.roll(row_masks(), -SHIFT))
    assert np.array_equal(np.roll(row_masks(), -SHIFT)[:5], row_masks()[SHIFT:SHIFT + 5])
    changed = np.zeros(R, bool)
    for name in want:
        changed |= (bits(want[name]) != bits(other[name])).reshape(R, -1).any(axis=1)
    print(kind, "rows that change:", int(changed.sum()), "of", R)
    assert changed.sum() >= (R + 3) // 4, (kind, int(changed.sum()))


# ---- the device ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    """One context for the file: the mixed frame, pseudonormal tables for both meshes, the object masks, and the tiling index."""
    import torch
    from pyrtx import api
    from test_gpu_query_signed import make_tables
    api.load_library()
    assert api.RTX_QUERY_CHUNK_RAYS == CHUNK
    sc, meshes = frame()
    r = api.Renderer(sc)
    keep = make_tables(r, meshes)
    r.set_object_masks(OBJECT_MASKS)
    idx = torch.arange(N, device="cuda") % R
    masks = torch.from_numpy(row_masks().view(np.int32)).cuda()[idx].contiguous()
    yield r, idx, masks
    del keep
    r.close()


def tiled(kind, idx):
    import torch
    return torch.from_numpy(base_rows(kind)).cuda()[idx].contiguous()


def check(got, kind, idx, names, what):
    """Tensors of `got` against the twin's base answers at i mod R, bit for bit, on the device."""
    import torch
    want = expected(kind)
    for name, key in names.items():
        g = got[name] if isinstance(got, dict) else got
        w = torch.from_numpy(bits(want[key])).cuda()[idx]
        g = g.view(torch.int32) if g.dtype == torch.float32 else g
        assert g.shape == w.shape, (what, name, tuple(g.shape), tuple(w.shape))
        bad = (g != w).reshape(N, -1).any(dim=1)
        assert not bool(bad.any()), (what, name, int(bad.sum()), torch.nonzero(bad)[:6].flatten().tolist())


@gpu
@pytest.mark.parametrize("sort", [False, True])
def test_nearest_reads_the_round_s_row_masks(ctx, sort):
    r, idx, masks = ctx
    got = r.query_nearest(tiled("nearest", idx), ("distance", "object_id"), mask=masks, sort=sort)
    check(got, "nearest", idx, {"distance": "distance", "object_id": "object_id"}, f"nearest sort {sort}")


@gpu
def test_signed_distance_writes_at_the_round_s_offset(ctx):
    r, idx, masks = ctx
    rows = tiled("signed", idx)
    got = r.query_signed_distance(rows, ("distance",), mask=masks, feature=True)
    check(got, "signed", idx, {"signed_distance": "signed_distance", "feature": "feature", "distance": "distance"}, "signed")
    alone = r.query_signed_distance(rows, (), mask=masks, feature=True)
    assert set(alone) == {"signed_distance", "feature"}
    check(alone, "signed", idx, {"signed_distance": "signed_distance", "feature": "feature"}, "signed, no channel")


@gpu
def test_hits_lists_k_entries_per_row_past_the_round(ctx):
    r, idx, masks = ctx
    rows = tiled("hits", idx)
    got = r.query_hits(rows, 2, ("distance", "triangle_id"), count=True, mask=masks)
    check(got, "hits", idx, {"distance": "distance", "triangle_id": "triangle_id", "count": "count"}, "hits K 2")
    check(r.query_hits(rows, 0, (), mask=masks), "hits", idx, {"count": "count"}, "hits count only")


@gpu
def test_sweep_reads_the_round_s_row_masks(ctx):
    r, idx, masks = ctx
    got = r.query_sweep(tiled("sweep", idx), ("distance", "object_id"), mask=masks)
    check(got, "sweep", idx, {"distance": "distance", "object_id": "object_id"}, "sweep")


@gpu
def test_overlap_lists_k_entries_per_row_past_the_round(ctx):
    r, idx, masks = ctx
    rows = tiled("overlap", idx)
    got = r.query_overlap(rows, 2, count=True, mask=masks)
    check(got, "overlap", idx, {"object_id": "object_id", "triangle_id": "triangle_id", "count": "count"}, "overlap K 2")
    check(r.query_overlapped(rows, mask=masks), "overlap", idx, {"any": "any"}, "overlapped")
