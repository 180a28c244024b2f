"""The frame the three walk queries share (k_query_nearest, k_query_hits, k_query_sweep: 256 lanes, tile after tile from one counter, rows staged
in LDS, the stack in LDS and the spill regions, the hit list in LDS, one sort block per context), where a row's answer could depend on what
the lane, the workgroup or the context did just before.  Every comparison is bit for bit (NaN == NaN) against the host twin's answers for the
same rows (the ray queries: the batch oracle), every row answered by the twin:
  * RTX_QUERY_GRID = 1, 2, 3: a workgroup walks its second to sixth tile with real work — hard sweeps, K = 8 lists with and without a count,
    the count-only form, every channel, a stack past RTX_LDS_STACK — sorted and unsorted, n a multiple of 256 and n with one row in the last tile;
    that the knob does cap the grid is read off the time of a 64-tile call, and bad values of it are ignored;
  * the same rows with their tiles in reverse order and dead tiles between dense ones: the same answers, permuted;
  * RTX_NEAREST_FETCH=0, the tiles-by-stride path of k_query_nearest: parity with the twin and equality with the counter path;
  * nearest, sweep, hits, closest, occluded and frames queued on one context without a wait, the sort block made, grown and reused in between;
  * two contexts on two scenes and two streams, queued alternately.
Row sets: the generators' rows of the kernels' own test files for as many seeds as the length needs (at least two), cut to 5 * 256 + 3 rows, so
that a row sits in another lane and wave in every tile."""
import numpy as np
import pytest

import hitset
import sweepset
import util
import test_gpu_query as Q
import test_gpu_query_hits as H
import test_gpu_query_nearest as N
import test_gpu_query_sweep as S
from test_gpu_query import check_channels, dev, host as to_host, same_bits
from test_gpu_query_hits import check
from test_gpu_rays import check_occ

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL = hitset.ALL
TILE = 256                                                                  # RTX_QUERY_BLOCK
LDS_STACK = 16                                                              # RTX_LDS_STACK
LONG = 5 * TILE + 3                                                         # six tiles, the last one ragged; not a multiple of 64
CASES = [("nearest", "materials_aniso"), ("nearest", "chain_blas"), ("sweep", "materials_aniso"), ("sweep", "chain_blas"),
         ("hits", "materials_aniso"), ("hits", "slab_chain"), ("hits", "quad_stack")]
_SETS = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def renderer(api, monkeypatch, sc, grid=None, fetch=None):
    """A fresh context: the knobs are read once, in rtx_create."""
    for knob, v in (("RTX_QUERY_GRID", grid), ("RTX_NEAREST_FETCH", fetch)):
        if v is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, str(v))
    return api.Renderer(sc)


def twin_answers(kind, sc, rows, blas=None):
    """The host twin on every row: nearest / sweep {channel: array, stack_max}; hits the same at K = 8 with the count, plus "no count": the
    lists of the call without a count (the shrinking bound).  sc: a scene, or with `blas` the arrays read_back() returns."""
    from pyrtx import host
    if kind == "nearest":
        return host.query_nearest(sc, rows, ALL, blas=blas)
    if kind == "sweep":
        return host.query_sweep(sc, rows, ALL, blas=blas)
    out = host.query_hits(sc, rows, 8, ALL, blas=blas)
    out["no count"] = host.query_hits(sc, rows, 8, ALL, count=False, blas=blas)
    out["no count"].pop("stack_max")
    return out


def row_set(kind, name, n=LONG):
    """(scene, rows (n, width), labels, twin answers): the rows of the kernel's own generated(name, seed) for seeds 4 apart, concatenated until
    n rows are there, then cut; once per run."""
    key = (kind, name, n)
    if key not in _SETS:
        module, first = {"nearest": (N, 31), "sweep": (S, 31), "hits": (H, 5)}[kind]
        parts, labels, k = [], [], 0
        while k < 2 or sum(len(p) for p in parts) < n:
            sc, rows, lab, _ = module.generated(name, seed=first + 4 * k)
            parts.append(rows); labels.append(lab); k += 1
        rows = np.ascontiguousarray(np.concatenate(parts)[:n])
        assert len(rows) == n and n % 64 != 0
        _SETS[key] = (sc, rows, np.concatenate(labels)[:n], twin_answers(kind, sc, rows))
    return _SETS[key]


def later_tiles_are_deep(kind, name, sc, rows, want):
    """What the deep scenes are here for, in the tiles after the first."""
    from pyrtx import host
    later = rows[TILE:]
    if name in ("chain_blas", "slab_chain"):
        assert want["stack_max"] > LDS_STACK
        deep = {"nearest": lambda: host.query_nearest(sc, later, "distance"), "sweep": lambda: host.query_sweep(sc, later, "distance"),
                "hits": lambda: host.query_hits(sc, later, 0, ())}[kind]()
        assert deep["stack_max"] > LDS_STACK, "no row after the first tile reaches the spill region"
    if name == "quad_stack":
        assert (want["count"][TILE:] > 8).sum() >= 24, "rows with more hits than the list holds, after the first tile"


def run(r, kind, rows_t, sort, n=None):
    """Every form of the kind's call -> {what: tensors}."""
    if kind == "nearest":
        return {"all channels": r.query_nearest(rows_t, ALL, n=n, sort=sort)}
    if kind == "sweep":
        return {"all channels": r.query_sweep(rows_t, ALL, n=n, sort=sort)}
    return {"K 8 with count": r.query_hits(rows_t, 8, ALL, n=n, sort=sort), "K 8 no count": r.query_hits(rows_t, 8, ALL, count=False, n=n, sort=sort),
            "count only": r.query_hits(rows_t, 0, (), n=n, sort=sort)}


def compare(kind, got, want, labels, what):
    for form, out in got.items():
        assert all(len(t) == len(next(iter(out.values()))) for t in out.values())
        if kind == "hits":
            assert tuple(out) == {"K 8 with count": ALL + ("count",), "K 8 no count": ALL, "count only": ("count",)}[form]
            check(out, want["no count"] if form == "K 8 no count" else want, labels, f"{what}, {form}")
        else:
            assert tuple(out) == ALL
            check_channels(out, want, labels, f"{what}, {form}")


# ---- 1. later tiles --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2, 3])
@pytest.mark.parametrize("kind,name", CASES)
def test_later_tiles_equal_the_host_walk(api, monkeypatch, kind, name, grid):
    """Six tiles over one, two or three workgroups: with one, tiles 1 .. 5 are later tiles of the same workgroup, in counter order."""
    sc, rows, labels, want = row_set(kind, name)
    assert (len(rows) + TILE - 1) // TILE >= 5
    later_tiles_are_deep(kind, name, sc, rows, want)
    r = renderer(api, monkeypatch, sc, grid)
    rows_t = dev(rows)
    state, blas = N.read_back(r, sc)
    back = twin_answers(kind, state, rows, blas)
    for sort in (False, True):
        got = run(r, kind, rows_t, sort)
        compare(kind, got, want, labels, f"{kind} {name} grid {grid} sort {sort}")
        compare(kind, got, back, labels, f"{kind} {name} grid {grid} sort {sort}, arrays read back")


@pytest.mark.parametrize("kind", ["nearest", "sweep", "hits"])
def test_a_full_last_tile_and_a_last_tile_of_one_row(api, monkeypatch, kind):
    sc, rows, labels, want = row_set(kind, "materials_aniso")
    rows_t = dev(rows)
    for grid in (1, 3):
        r = renderer(api, monkeypatch, sc, grid)
        for n in (5 * TILE, 5 * TILE + 1):
            for sort in (False, True):
                got = run(r, kind, rows_t, sort, n=n)
                assert all(len(t) == n for out in got.values() for t in out.values())
                compare(kind, got, want, labels, f"{kind} grid {grid} n {n} sort {sort}")


def test_invalid_grid_values_are_ignored(api, monkeypatch, capfd):
    sc, rows, labels, want = row_set("hits", "materials_aniso")
    rows_t = dev(rows)
    for bad in ("-3", "banana", "2.5", str(2 ** 40)):
        capfd.readouterr()
        r = renderer(api, monkeypatch, sc, bad)
        assert f"RTX_QUERY_GRID={bad} ignored" in capfd.readouterr().err
        compare("hits", run(r, "hits", rows_t, False), want, labels, f"RTX_QUERY_GRID={bad}")
    capfd.readouterr()
    renderer(api, monkeypatch, sc, 0)
    renderer(api, monkeypatch, sc, 1)
    assert "RTX_QUERY_GRID" not in capfd.readouterr().err


@pytest.mark.parametrize("kind", ["nearest", "sweep", "hits"])
def test_the_grid_cap_is_honoured(api, monkeypatch, kind):
    """Nothing the ABI returns says how many workgroups a call launched; its time does.  2^14 rows are 64 tiles: without a cap they run
    side by side on 64 compute units (the spill region is sized for the persistent grids of the traversal kernels, hundreds of workgroups),
    with RTX_QUERY_GRID=1 one workgroup on one compute unit walks them one after the other — up to 64 times the time, less what a launch
    costs.  Asserted: 4 times, the best of three calls each, so that the tests above can be trusted to run later tiles.  The answers are
    the same."""
    import torch
    sc, rows, labels, want = row_set(kind, "materials_aniso")
    n = 2 ** 14
    big = dev(rows).repeat((n + len(rows) - 1) // len(rows), 1)[:n].contiguous()

    def call(r):
        if kind == "hits":
            return r.query_hits(big, 0, ())["count"]
        return (r.query_nearest if kind == "nearest" else r.query_sweep)(big, ("distance",))["distance"]

    def best_ms(r):
        out = call(r)                                                   # the first call makes the counter and moves the context to a stream
        times = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = call(r); b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return min(times), out

    full_ms, full = best_ms(renderer(api, monkeypatch, sc))
    one_ms, one = best_ms(renderer(api, monkeypatch, sc, 1))
    print(f"{kind}: {n} rows, no cap {full_ms:.3f} ms, RTX_QUERY_GRID=1 {one_ms:.3f} ms, ratio {one_ms / full_ms:.0f}")
    assert torch.equal(full.view(torch.int32), one.view(torch.int32))
    assert one_ms > 4 * full_ms, (kind, full_ms, one_ms)


# ---- 2. order independence -------------------------------------------------------------------------------------------------------------
def dead_rows(kind, rows, count):
    """`count` rows that are no query, each a live row of the set made dead: a lane that walked one anyway would find that row's answer.
    In turn a zero direction (nearest has none: a NaN maximum distance), a NaN origin, a maximum distance of 0 and a negative one."""
    out = rows[np.arange(count) % len(rows)].copy()
    far = 3 if kind == "nearest" else 6
    for j in range(count):
        how = j % 4
        if how == 0:
            if kind == "nearest":
                out[j, 3] = np.nan
            else:
                out[j, 3:6] = (0.0, -0.0, 0.0)
        elif how == 1:
            out[j, j % 3] = np.nan
        else:
            out[j, far] = 0.0 if how == 2 else -2.0
    return out


def is_dead(kind, rows):
    if kind == "nearest":
        with np.errstate(invalid="ignore"):
            return ~(np.isfinite(rows[:, :3]).all(axis=1) & (rows[:, 3] > 0))
    return hitset.is_dead(rows) if kind == "hits" else ~sweepset.is_live(rows)


def permuted(kind, rows):
    """(rows of every tile in reverse tile order, source row of each or -1): the ragged tile comes first, padded to a tile with dead rows; after
    the first dense tile stands a tile of dead rows alone."""
    tiles = [np.arange(b, min(b + TILE, len(rows))) for b in range(0, len(rows), TILE)][::-1]
    src = []
    for j, t in enumerate(tiles):
        src += [t, np.full(TILE - len(t), -1)]
        if j == 1:
            src.append(np.full(TILE, -1))
    src = np.concatenate(src)
    out = dead_rows(kind, rows, len(src))
    out[src >= 0] = rows[src[src >= 0]]
    return np.ascontiguousarray(out), src


def no_answer(name, shape, dtype):
    return np.full(shape, np.inf if name == "distance" else 0 if name in ("position", "normal", "uv", "count") else -1, dtype)


@pytest.mark.parametrize("kind,name", CASES)
def test_tiles_in_reverse_order_with_dead_tiles_between(api, monkeypatch, kind, name):
    sc, rows, labels, want = row_set(kind, name)
    perm, src = permuted(kind, rows)
    live = src >= 0
    assert len(perm) == 7 * TILE and is_dead(kind, perm[~live]).all() and not live[2 * TILE:3 * TILE].any() and live[TILE:2 * TILE].all() and live[3 * TILE:].all()
    # the twin on the permuted rows: the same rows' answers, permuted, and the no-answer record for the dead ones
    ref = twin_answers(kind, sc, perm)
    for group, base in ((ref, want),) + (((ref["no count"], want["no count"]),) if kind == "hits" else ()):
        for ch, a in group.items():
            if ch in ("stack_max", "no count"):
                continue
            assert same_bits(a[live], base[ch][src[live]]).all(), ch
            assert same_bits(a[~live], no_answer(ch, a[~live].shape, a.dtype)).all(), ch
    perm_t = dev(perm)
    for grid in (1, None):
        r = renderer(api, monkeypatch, sc, grid)
        for sort in (False, True):
            compare(kind, run(r, kind, perm_t, sort), ref, None, f"{kind} {name} permuted, grid {grid} sort {sort}")


# ---- 3. tiles by stride ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [None, 1, 3])
@pytest.mark.parametrize("name", ["materials_aniso", "chain_blas"])
def test_tiles_by_stride_equal_the_twin_and_the_counter_path(api, monkeypatch, name, grid):
    import torch
    sc, rows, labels, want = row_set("nearest", name)
    later_tiles_are_deep("nearest", name, sc, rows, want)
    counter = renderer(api, monkeypatch, sc, grid)
    stride = renderer(api, monkeypatch, sc, grid, fetch=0)
    rows_t = dev(rows)
    for n in (LONG, 5 * TILE, 5 * TILE + 1):
        for sort in (False, True):
            a = counter.query_nearest(rows_t, ALL, n=n, sort=sort)
            b = stride.query_nearest(rows_t, ALL, n=n, sort=sort)
            check_channels(b, want, labels, f"{name} by stride, grid {grid} n {n} sort {sort}")
            for ch in ALL:
                assert torch.equal(a[ch].view(torch.int32), b[ch].view(torch.int32)), (name, grid, n, sort, ch)


# ---- 4. mixed calls on one context, no wait --------------------------------------------------------------------------------------------
def out_tensors(api, n, hits=0, count=False):
    import torch
    out = {}
    for name, (_, dt, k) in api.QUERY_CHANNELS.items():
        shape = (n,) + ((hits,) if hits else ()) + ((k,) if k > 1 else ())
        out[name] = torch.full(shape, -77, dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda")
    if count:
        out["count"] = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    return out


@pytest.mark.parametrize("grid", [None, 1])
def test_mixed_calls_on_one_context_without_a_wait(api, monkeypatch, grid):
    """nearest, sweep, hits, closest, occluded and two frames on one stream with one wait at the end, twice: the tile counter and the spill
    regions shared with the closest-hit launches, one sort block for rows of 4, 8, 7, 6 and 7 floats that the second call grows."""
    import torch
    sc, pts, _, want_n = row_set("nearest", "materials_aniso")
    _, sweeps, _, want_s = row_set("sweep", "materials_aniso")
    _, segs, _, want_h = row_set("hits", "materials_aniso")
    _, rays, dist, ray_labels, want_c, want_o = Q.generated("materials_aniso")
    occ_rows = Q.segments_of(rays, dist)
    assert 300 < len(occ_rows) and len(rays) < LONG
    monkeypatch.delenv("RTX_QUERY_GRID", raising=False)
    ref = api.Renderer(sc).render()                                     # a context that only renders
    r = renderer(api, monkeypatch, sc, grid)
    pts_t, sweeps_t, segs_t, rays_t, occ_t = dev(pts), dev(sweeps), dev(segs), dev(rays), dev(occ_rows)
    rgb = torch.zeros((sc.height, sc.width, 3), dtype=torch.float32, device="cuda")
    packed = torch.zeros((sc.height, sc.width), dtype=torch.int32, device="cuda")
    r.bind_framebuffer(rgb.data_ptr(), packed.data_ptr())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for again in (False, True):                                         # the second pass is the steady state: nothing is made or grown
        done, frames = [], []

        def nearest(n, sort):
            done.append((f"nearest n {n} sort {sort}", r.query_nearest(pts_t, ALL, out=out_tensors(api, n), n=n, sort=sort), want_n, check_channels))

        def sweep(sort):
            done.append((f"sweep sort {sort}", r.query_sweep(sweeps_t, ALL, out=out_tensors(api, LONG), sort=sort), want_s, check_channels))

        def hits(sort):
            done.append((f"hits sort {sort}", r.query_hits(segs_t, 8, ALL, out=out_tensors(api, LONG, 8, True), sort=sort), want_h, check))

        def closest(sort):
            done.append((f"closest sort {sort}", r.query_closest(rays_t, ALL, out=out_tensors(api, len(rays)), sort=sort), want_c, check_channels))

        def occluded(sort):
            done.append((f"occluded sort {sort}", r.query_occluded(occ_t, out=torch.full((len(occ_rows),), -77, dtype=torch.int32, device="cuda"), sort=sort), None, None))

        def frame():
            r.render_async()
            frames.append((rgb.clone(), packed.clone()))                # on the stream the frame was queued on

        with torch.cuda.stream(side):
            nearest(300, True)                                          # the first sorted call of the context makes the sort block
            sweep(True)                                                 # more rows: the block grows
            hits(True); closest(True); occluded(True)
            frame()
            occluded(False); closest(False); hits(False); sweep(False); nearest(300, False)
            nearest(65, True)                                           # fewer rows than the block holds
            frame()
        torch.cuda.synchronize()                                        # the one wait
        assert len(done) == 11 and len(frames) == 2
        for what, got, want, checker in done:
            if checker is None:
                check_occ(to_host(got).reshape(dist.shape) != 0, want_o, ray_labels)
            else:
                checker(got, want, None, f"{what}, pass {1 + again}, grid {grid}")
        stats, _ = r.stats()
        assert stats == ref["stats"]
        for k, (f_rgb, f_packed) in enumerate(frames):
            assert util.bit_exact(to_host(f_rgb), ref["rgb"]) and np.array_equal(to_host(f_packed).view(np.uint32), ref["packed"]), (k, again)
    r.close()                                                           # before the framebuffer tensors go


# ---- 5. two contexts -------------------------------------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_answer_for_their_own_scene(api, monkeypatch):
    import torch
    names = ("materials_aniso", "chain_blas")
    sets = {(kind, name): row_set(kind, name) for kind in ("nearest", "sweep", "hits") for name in names}
    ctx = {name: renderer(api, monkeypatch, sets[("nearest", name)][0]) for name in names}
    streams = {name: torch.cuda.Stream() for name in names}
    rows_t = {key: dev(s[1]) for key, s in sets.items()}
    torch.cuda.synchronize()
    done = []
    for sort in (False, True):
        for kind in ("nearest", "sweep", "hits"):
            for name in names:                                          # the two contexts take turns
                with torch.cuda.stream(streams[name]):
                    done.append((kind, name, sort, run(ctx[name], kind, rows_t[(kind, name)], sort)))
    torch.cuda.synchronize()
    for kind, name, sort, got in done:
        compare(kind, got, sets[(kind, name)][3], sets[(kind, name)][2], f"{kind} on {name}, sort {sort}, two contexts")
    # the two scenes do answer differently: the same rows on the other context
    other = ctx["chain_blas"].query_nearest(rows_t[("nearest", "materials_aniso")], ("distance",))
    assert not same_bits(to_host(other["distance"]), sets[("nearest", "materials_aniso")][3]["distance"]).all()
