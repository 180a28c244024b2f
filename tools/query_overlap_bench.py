"""Mrows/s of the box-overlap queries (Renderer.query_overlap / query_overlapped: rows and answers in device tensors, queued on a torch
stream), in the shape of tools/query_sweep_bench.py.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces): 255 296 triangles, one instance
  (a) grid  a 128^3 voxel grid over the scene's bounds (api.grid_boxes, x fastest: 2 097 152 axis-aligned rows per call)
              any       query_overlapped: 0 / 1 per voxel, the occupancy grid
              count     query_overlap(max_hits=0): the triangles per voxel
              objects   query_overlap(max_hits=4, objects=True) with its count
              nearest   what the library offered before: query_nearest on the voxel centres with rmax = the half diagonal, distance only.  It
                        answers a larger question (a ball, not a box): the ratio is context, not a threshold
  (b) boxes 2^20 randomly oriented boxes of about 1e-2 of the scene's size, centred within three box sizes of a random surface point
              k4        query_overlap(max_hits=4) with its count, rows in generation order (incoherent)
              k4_sorted the same rows with sort=True (RTX_QUERY_SORT): what the library's own sort buys, its cost included

Timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants
alternate within each of `--rounds` rounds, the medians are reported.  Checked first: any == (count > 0) on the grid, sorted == unsorted.

  python tools/query_overlap_bench.py --out profiles/query_overlap_bench.json
  python tools/query_overlap_bench.py --mask rows      the filtered calls: none (default), ones, half, rows — tools/query_masks.py
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

VARIANTS = ("any", "count", "objects", "nearest", "k4", "k4_sorted")
GRID = 128

import query_masks  # noqa: E402


def surface_boxes(sc, n, size, seed=2026):
    """n boxes (n, 10): half extents 1e-2 * size * U(0.5, 1.5), a random unit quaternion, centred within three box sizes of a point drawn
    from a random triangle of the scene (world space)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    inst = rng.integers(len(sc.instances), size=n)
    rows = np.zeros((n, 10), np.float32)
    for k, I in enumerate(sc.instances):
        sel = np.flatnonzero(inst == k)
        hot = sc.blas[int(I["blas_id"])].tri_hot
        t = rng.integers(len(hot), size=len(sel))
        u = rng.uniform(0, 1, (len(sel), 2)); flip = u.sum(axis=1) > 1; u[flip] = 1 - u[flip]
        p = hot["position_0"][t].astype(np.float64) + hot["position_edge_1"][t] * u[:, :1] + hot["position_edge_2"][t] * u[:, 1:]
        m = np.asarray(I["world"], np.float64).reshape(4, 4)
        rows[sel, :3] = p @ m[:3, :3].T + m[:3, 3]
    h = 1e-2 * size * rng.uniform(0.5, 1.5, (n, 3))
    rows[:, 3:6] = h
    rows[:, :3] += rng.uniform(-3, 3, (n, 3)) * h
    q = rng.normal(size=(n, 4))
    rows[:, 6:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="write the rows and medians as JSON here")
    query_masks.add_argument(ap)
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyrtx import api, host
    import pointset
    assert torch.cuda.is_available(), "query_overlap_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    lo, hi = pointset.world_box(sc)
    size = float(np.max(hi - lo))
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    cell = (hi - lo) / GRID
    grid = api.grid_boxes(lo, cell, (GRID, GRID, GRID), device="cuda")
    ng, nb = len(grid), 1 << 20
    boxes = torch.from_numpy(surface_boxes(sc, nb, size)).cuda()
    centres = torch.cat([grid[:, :3], torch.full((ng, 1), float(np.linalg.norm(0.5 * cell)), dtype=torch.float32, device="cuda")], dim=1).contiguous()
    mask_g = query_masks.setup(r, sc, args.mask, ng)                     # --mask: the filtered calls (tools/query_masks.py)
    mask_b = query_masks.setup(r, sc, args.mask, nb)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    out_any, out_count, out_obj = i32(ng), i32(ng), {"object_id": i32(ng, 4), "count": i32(ng)}
    out_k4 = {"object_id": i32(nb, 4), "triangle_id": i32(nb, 4), "count": i32(nb)}
    dist = torch.empty((ng,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def call(variant):
        if variant == "any":
            r.query_overlapped(grid, out=out_any, mask=mask_g)
        elif variant == "count":
            r.query_overlap(grid, 0, out={"count": out_count}, mask=mask_g)
        elif variant == "objects":
            r.query_overlap(grid, 4, objects=True, out=out_obj, mask=mask_g)
        elif variant == "nearest":
            r.query_nearest(centres, ("distance",), out={"distance": dist}, mask=mask_g)
        else:
            r.query_overlap(boxes, 4, out=out_k4, sort=variant == "k4_sorted", mask=mask_b)
        return ng if variant in ("any", "count", "objects", "nearest") else nb

    def timed(variant):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call(variant)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                n = call(variant)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps, n

    # a rate of wrong answers is no rate
    with torch.cuda.stream(stream):
        for v in ("any", "count", "objects", "nearest", "k4"):
            call(v)
    stream.synchronize()
    assert torch.equal(out_any, (out_count > 0).to(torch.int32)) and torch.equal(out_any, (out_obj["count"] > 0).to(torch.int32))
    occupied, within_ball = int(out_any.sum()), int(torch.isfinite(dist).sum())
    assert within_ball >= occupied                                      # the ball of the half diagonal holds the voxel
    plain = {k: t.clone() for k, t in out_k4.items()}
    with torch.cuda.stream(stream):
        call("k4_sorted")
    stream.synchronize()
    for k, t in out_k4.items():
        assert torch.equal(t, plain[k]), k
    answered, full = int((plain["count"] > 0).sum()), int((plain["count"] > 4).sum())
    results = []
    for rnd in range(args.rounds):
        for variant in VARIANTS:
            ms, n = timed(variant)
            row = {"variant": variant, "round": rnd, "rows": n, "ms_per_call": ms, "mrows_per_s": n / ms / 1e3}
            results.append(row)
            print(json.dumps(row), flush=True)
    summary = {}
    for row in results:
        summary.setdefault(row["variant"], []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    ratios = {f"{v}_over_nearest": summary[v]["median_mrows_per_s"] / summary["nearest"]["median_mrows_per_s"] for v in ("any", "count", "objects")}
    ratios["any_over_count"] = summary["any"]["median_mrows_per_s"] / summary["count"]["median_mrows_per_s"]
    ratios["k4_sorted_over_k4"] = summary["k4_sorted"]["median_mrows_per_s"] / summary["k4"]["median_mrows_per_s"]
    facts = {"grid": GRID, "voxels": ng, "voxels_occupied": occupied, "voxel_centres_within_the_half_diagonal": within_ball, "boxes": nb, "boxes_with_an_overlap": answered,
             "boxes_with_more_than_4": full}
    res = {"tool": "tools/query_overlap_bench.py", "scene": "atrium stand-in 1920x1080", "scene_size": size, "steps": args.steps, "rounds": args.rounds, "mask": args.mask,
           **facts, "summary": summary, "ratios": ratios, "rows": results}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"ratios": ratios, **facts}, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
