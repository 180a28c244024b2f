"""Mrows/s of the capsule-overlap queries (Renderer.query_overlap_capsule / query_overlapped_capsule: rows and answers in device tensors,
queued on a torch stream), in the shape of tools/query_overlap_bench.py.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces): 255 296 triangles, one instance
  rows      2^20 capsules near surfaces: the start point within three capsule sizes of a random surface point, the axis a random direction
            of 1e-2 * U(1, 3) of the scene's size, r = 1e-2 * U(0.25, 0.75) of it; rows in generation order (incoherent)
              any          query_overlapped_capsule: 0 / 1 per row
              count        query_overlap_capsule(max_hits=0)
              objects      query_overlap_capsule(max_hits=4, objects=True) with its count
              k4           query_overlap_capsule(max_hits=4) with its count
              k4_sorted    the same with sort=True (RTX_QUERY_SORT, the ray key over start point and axis), its cost included (--sort: every
                           variant sorted)
              balls        k4 on the same rows with the axis set to 0: the within-radius gather
            and, on the same rows, the substitutes this query replaces:
              box_k4       query_overlap(max_hits=4) with each capsule's bounding oriented box (centre the axis' midpoint, half extents
                           (|d| / 2 + r, r, r), turned so that x lies along the axis): a larger question
              sweep        query_sweep along the axis (origin, d / |d|, |d|, r), distance only: against `any`

Timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants
alternate within each of `--rounds` rounds, the medians are reported.  Checked first: any == (count > 0) == (objects count > 0),
sorted == unsorted, every capsule that overlaps is found by its bounding box.

  python tools/query_overlap_capsule_bench.py --out profiles/query_overlap_capsule_bench.json
  python tools/query_overlap_capsule_bench.py --mask rows      the filtered calls: none (default), ones, half, rows — tools/query_masks.py
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

VARIANTS = ("any", "count", "objects", "k4", "k4_sorted", "balls", "box_k4", "sweep")

import query_masks  # noqa: E402


def surface_capsules(sc, n, size, seed=2026):
    """n capsules (n, 7) near surfaces, and their bounding oriented boxes (n, 10) and sweeps (n, 8)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    inst = rng.integers(len(sc.instances), size=n)
    p = np.zeros((n, 3))
    for k, I in enumerate(sc.instances):
        sel = np.flatnonzero(inst == k)
        hot = sc.blas[int(I["blas_id"])].tri_hot
        t = rng.integers(len(hot), size=len(sel))
        u = rng.uniform(0, 1, (len(sel), 2)); flip = u.sum(axis=1) > 1; u[flip] = 1 - u[flip]
        q = hot["position_0"][t].astype(np.float64) + hot["position_edge_1"][t] * u[:, :1] + hot["position_edge_2"][t] * u[:, 1:]
        m = np.asarray(I["world"], np.float64).reshape(4, 4)
        p[sel] = q @ m[:3, :3].T + m[:3, 3]
    r = 1e-2 * size * rng.uniform(0.25, 0.75, n)
    length = 1e-2 * size * rng.uniform(1.0, 3.0, n)
    a = rng.normal(size=(n, 3)); a /= np.linalg.norm(a, axis=1, keepdims=True)
    p += rng.uniform(-3, 3, (n, 3)) * r[:, None]
    caps = np.concatenate([p, a * length[:, None], r[:, None]], axis=1).astype(np.float32)
    # the quaternion that turns x onto a: axis x cross a, angle acos(a.x); (1 + a.x, 0, -a.z, a.y) normalised, (0, 0, 1, 0) for a = -x
    q = np.stack([np.zeros(n), -a[:, 2], a[:, 1], 1.0 + a[:, 0]], axis=1)
    q[np.linalg.norm(q, axis=1) < 1e-6] = (0.0, 0.0, 1.0, 0.0)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    boxes = np.concatenate([p + 0.5 * a * length[:, None], (0.5 * length + r)[:, None], r[:, None], r[:, None], q], axis=1).astype(np.float32)
    sweeps = np.concatenate([p, a, length[:, None], r[:, None]], axis=1).astype(np.float32)
    return caps, boxes, sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sort", action="store_true", help="every capsule variant with RTX_QUERY_SORT")
    ap.add_argument("--out", help="write the rows and medians as JSON here")
    query_masks.add_argument(ap)
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyrtx import api, host
    import pointset
    assert torch.cuda.is_available(), "query_overlap_capsule_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    lo, hi = pointset.world_box(sc)
    size = float(np.max(hi - lo))
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    n = 1 << 20
    caps_h, boxes_h, sweeps_h = surface_capsules(sc, n, size)
    caps, boxes, sweeps = (torch.from_numpy(x).cuda() for x in (caps_h, boxes_h, sweeps_h))
    balls = caps.clone(); balls[:, 3:6] = 0.0
    mask = query_masks.setup(r, sc, args.mask, n)                        # --mask: the filtered calls (tools/query_masks.py)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    out_any, out_count, out_obj = i32(n), i32(n), {"object_id": i32(n, 4), "count": i32(n)}
    out_k4 = {"object_id": i32(n, 4), "triangle_id": i32(n, 4), "count": i32(n)}
    out_ball = {"object_id": i32(n, 4), "triangle_id": i32(n, 4), "count": i32(n)}
    out_box = {"object_id": i32(n, 4), "triangle_id": i32(n, 4), "count": i32(n)}
    dist = torch.empty((n,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def call(variant):
        s = args.sort
        if variant == "any":
            r.query_overlapped_capsule(caps, out=out_any, mask=mask, sort=s)
        elif variant == "count":
            r.query_overlap_capsule(caps, 0, out={"count": out_count}, mask=mask, sort=s)
        elif variant == "objects":
            r.query_overlap_capsule(caps, 4, objects=True, out=out_obj, mask=mask, sort=s)
        elif variant == "balls":
            r.query_overlap_capsule(balls, 4, out=out_ball, mask=mask, sort=s)
        elif variant == "box_k4":
            r.query_overlap(boxes, 4, out=out_box, mask=mask, sort=s)
        elif variant == "sweep":
            r.query_sweep(sweeps, ("distance",), out={"distance": dist}, mask=mask, sort=s)
        else:
            r.query_overlap_capsule(caps, 4, out=out_k4, sort=s or variant == "k4_sorted", mask=mask)

    def timed(variant):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call(variant)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                call(variant)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    # a rate of wrong answers is no rate
    with torch.cuda.stream(stream):
        for v in ("any", "count", "objects", "k4", "balls", "box_k4", "sweep"):
            call(v)
    stream.synchronize()
    assert torch.equal(out_any, (out_count > 0).to(torch.int32)) and torch.equal(out_any, (out_obj["count"] > 0).to(torch.int32)) and torch.equal(out_k4["count"], out_count)
    # the box holds the capsule and the capsule its start ball, but for pairs within rounding of touching.  Flags, not counts: this mesh has
    # split leaves, where a count is one of slots found and depends on the volume's extent
    assert int(((out_box["count"] > 0) < (out_count > 0)).sum()) * 10000 <= n, "capsules overlap where their bounding boxes do not"
    assert int(((out_ball["count"] > 0) > (out_count > 0)).sum()) * 10000 <= n, "start balls overlap where their capsules do not"
    plain = {k: t.clone() for k, t in out_k4.items()}
    with torch.cuda.stream(stream):
        call("k4_sorted")
    stream.synchronize()
    for k, t in out_k4.items():
        assert torch.equal(t, plain[k]), k
    swept = torch.isfinite(dist)
    facts = {"rows": n, "rows_with_an_overlap": int(out_any.sum()), "rows_with_more_than_4": int((out_count > 4).sum()), "mean_count": float(out_count.float().mean()),
             "boxes_with_an_overlap": int((out_box["count"] > 0).sum()), "mean_box_count": float(out_box["count"].float().mean()),
             "balls_with_an_overlap": int((out_ball["count"] > 0).sum()), "sweeps_with_a_contact": int(swept.sum()),
             "sweep_and_any_differ": int((swept != (out_any > 0)).sum())}
    results = []
    for rnd in range(args.rounds):
        for variant in VARIANTS:
            ms = timed(variant)
            row = {"variant": variant, "round": rnd, "rows": n, "ms_per_call": ms, "mrows_per_s": n / ms / 1e3}
            results.append(row)
            print(json.dumps(row), flush=True)
    summary = {}
    for row in results:
        summary.setdefault(row["variant"], []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    med = lambda v: summary[v]["median_mrows_per_s"]
    ratios = {"k4_over_box_k4": med("k4") / med("box_k4"), "any_over_sweep": med("any") / med("sweep"), "k4_sorted_over_k4": med("k4_sorted") / med("k4"),
              "balls_over_k4": med("balls") / med("k4"), "any_over_count": med("any") / med("count")}
    res = {"tool": "tools/query_overlap_capsule_bench.py", "scene": "atrium stand-in 1920x1080", "scene_size": size, "steps": args.steps, "rounds": args.rounds, "mask": args.mask,
           "sort": bool(args.sort), **facts, "summary": summary, "ratios": ratios, "rows_timed": results}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"ratios": ratios, **facts}, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
